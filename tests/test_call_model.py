"""CPU tests of tests/call_model.py: the committed sequences of tests/test_call_sequences_gpu.py reach the histories they are there
for, and the model says what include/meao.h says (hand-written sequences, expectations typed in from the header -- so that a model
bug cannot cancel a library bug of the same shape)."""
import dataclasses
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
    if component == "mixed":                    # exactly what was announced, through the extents call with one frame smaller
        e = c.execute_extents(call["bufs"], call["outs"], ((384, 256, 1, 0), (200, 120, 1, 0)), params=call["params"], stream=0)
    else:
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
    # the dynamic-resolution sequences, computed with the generator as it was before it learnt mixed-size batches
    "dyn_stepped/r8_rtz_f32": "b63680cc0e484405e7037df2df784bda30871ad2997fbf5c83283254b4e2c788",
    "dyn_stepped/f16_rtne_unorm16": "3e546a97d7d5e49f950589833f790541a5ee2542fcde85b033faf4940841e639",
    "dyn_stepped/r8_rtz_linear_f32": "0cd951a3ab9a3be4474a63759ea5f3cc8e7a91a0785f1221ef178aeca9e85d4f",
    "dyn_stepped/r8_rtz_hq2": "955dab6ec8347739d9d55f42c7cfbd00df440812212c3694a09e134e9db2d96d",
    "dyn_stepped/r8_rtz_not_pipelined": "e7893446a622c282a8f75245695d08d80000b38afcd75d2b2439fcff3498beec",
    "dyn_free/r8_rtz_f32": "e954afdcb26a00b4605d8113188285d7b945199dca6bfd73a80eab27d87742fc",
    "dyn_free/r8_rtz_linear_f32": "8e6d0206465b78f2c6668dae2c95493c3a35e919791e0e8e1984422c42b98b25",
    "dyn_free/f16_rtne_unorm16": "91e7cde6e445e9b5dcca9d2e21bc63876183c23dc696ddb71488db04a48fd746",
    "dyn_pool_stepped/pool2": "36d31b5ac7f3502a8880c44702447a333a531c4c47584ba9eb2fce864070cd4d",
    "dyn_pool_stepped/pool3": "6b1388b2f47ab1fc1d08a5c70516678ff7dbfb3b102a69f09e13e3d391da4ddd",
    "dyn_pool_free/pool2": "97730b7be043aae6bf92032434178ebfa602f427a239e6b21940717cdbb02508",
    "dyn_pool_free/pool3": "f21e9e2ce79627065d0d6fc982787ddf593fbe8c8e567a00c1f7617c08fa40a3",
}


def test_older_sequences_are_what_they_were():
    import hashlib
    from tests import test_dynamic_resolution_sequences_gpu as D
    got = {"%s/%s" % (kind, name): M.case_sequence(kind, name)[0] for kind, name in M.committed_sequences() + M.dynamic_sequences()}
    assert not any(op.extents is not None for ops in got.values() for op in ops)     # (Op.extents is not in the repr)
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


# ---- mixed-size batches: the committed seeds of the new cases reach every rule

REQUIRED_MIXED = [
    "mixed_flushes_composite", "mixed_consumes_ready", "mixed_consumes_ready_same_buffers", "mixed_carries_plain",
    "mixed_carries_pitched", "mixed_carries_per_frame", "mixed_carries_sized", "mixed_carries_more_frames_than_n",
    "mixed_shared_params_takes_ring_slot", "sized_ready_from_mixed_kept_by_resize", "uniform_extents_reuses",
    "uniform_extents_carries", "mixed_refused_keeps_announcement", "mixed_refused_keeps_ready", "mixed_refused_keeps_composite",
    "mixed_then_debug_read", "mixed_then_reserve_invalidates", "mixed_after_invalidation", "mixed_on_other_stream",
    "pool_member_uniform_while_other_mixed", "pool_mixed_idle_member", "pool_mixed_refused_whole",
] + ["invalid_" + what for what in M.MIXED_INVALID]


@pytest.fixture(scope="module")
def mixed():
    total = Counter()
    per_case = {}
    for kind, name in M.mixed_sequences():
        ops, model = M.case_sequence(kind, name)
        per_case[(kind, name)] = Counter(M.events_of(ops, model))
        total += per_case[(kind, name)]
    return total, per_case


@pytest.mark.parametrize("event", REQUIRED_MIXED)
def test_mixed_sequences_reach(mixed, event):
    total, _ = mixed
    assert total[event] >= 2, (event, total[event])       # more than once: no rule rests on a single operation of a single seed


def test_every_mixed_case_carries_consumes_and_refuses(mixed):
    """Each case on its own: mixed calls that carry an announcement, one that consumes a ready set, one that is refused."""
    _, per_case = mixed
    for case, ev in per_case.items():
        assert ev["mixed_call"] >= 8 and ev["mixed_consumes_ready"] and ev["uniform_extents"], (case, ev["mixed_call"])
        assert sum(ev["mixed_carries_" + k] for k in ("plain", "pitched", "per_frame", "sized")) >= 3, case
        assert sum(ev["invalid_" + what] for what in M.MIXED_INVALID) >= 1, case


def test_mixed_sequences_are_deterministic_and_legal():
    for kind, name in M.mixed_sequences():
        a, model = M.case_sequence(kind, name)
        b, _ = M.case_sequence(kind, name)
        assert a == b
        M.replay(a, model)                      # the model asserts legality: refills, refused calls held to the rule they name
        assert sum(op.kind != "refill" for op in a) >= 40 and sum(op.kind == "execute" for op in a) >= 12, (kind, name)
        one = M.fresh_model(M.case_profile(kind, name)[1], M.case_profile(kind, name)[0])
        laid = {}
        for op in a:
            c = one.members[0] if kind.startswith("mix_pool") else one
            cur, cap = (c.width, c.height), c.capacity()
            if op.kind == "refill":
                laid.update({x: (op.size or cur, op.pitch) for x in op.bufs})
            if op.kind == "execute" and op.extents is not None:
                assert not (op.depth_host or op.out_host) and len(op.extents) == len(op.bufs) == len(op.outs), (kind, name, op)
                assert all(s[:2] in M.MIX_SIZES and s[0] <= cap[0] and s[1] <= cap[1] for s in op.extents), (kind, name, op)
                if not c.extents_uniform(op.extents) and not kind.startswith("mix_pool"):
                    assert any(s[:2] != cur for s in op.extents) or len({s[2:] for s in op.extents}) > 1, (kind, name, op)
            if op.kind == "comp_enqueue":
                # a composite reads AO surfaces packed at the context's size: after a mixed call only such frames are named
                last = [x for x in a[:a.index(op)] if x.kind == "execute"][-1]
                if last.extents is not None:
                    for o in op.bufs:
                        assert last.extents[last.outs.index(o)][:2] == cur and last.extents[last.outs.index(o)][3] == 0, (kind, name, op)
            one.apply(op)


def test_free_running_mixed_sequences_hold_nothing_that_synchronises():
    for kind, name in M.mixed_sequences():
        if kind not in ("mix_free", "mix_pool_free"):
            continue
        ops, model = M.case_sequence(kind, name)
        one = model.members[0] if kind == "mix_pool_free" else model
        assert one.cap == M.DYN_RESERVE
        for op in ops:
            assert op.kind != "reserve" and not (op.kind == "invalid" and op.on == "reserve"), (kind, name, op)
            assert not (op.depth_host or op.out_host or op.read_debug), (kind, name, op)
            if op.kind == "resize":
                assert one.within(*op.size) and one.cap == M.DYN_RESERVE, (kind, name, op)
            model.apply(op)


def test_replay_of_a_mixed_sequence_equals_the_generators_own_model():
    """generate() keeps a model of its own; replay(ops, fresh model) must walk through the same states: same events, same totals."""
    for kind, name in M.mixed_sequences():
        a, model = M.case_sequence(kind, name)
        b, again = M.case_sequence(kind, name)
        ea = [(op.kind, e if isinstance(e, list) else [e]) for op, e in M.replay(a, model)]
        eb = [(op.kind, e if isinstance(e, list) else [e]) for op, e in M.replay(b, again)]
        assert ea == eb
        assert all(x is None or x.status == (M.ERR_INVALID_ARGUMENT if k == "invalid" else M.OK) for k, e in ea for x in e), (kind, name)
        members = model.members if kind.startswith("mix_pool") else [model]
        assert sum(m.totals["mixed"] for m in members) == sum("mixed_call" in x.events for _, e in ea for x in e if x is not None)


# ---- mixed-size batches: the model against the header, by hand

MIXED2 = ((384, 256, 0, 0), (200, 120, 0, 0))


def test_a_mixed_call_is_a_per_frame_call_also_without_params():
    """'Every other call is a "mixed call", a per-frame call (it reads its argument blocks from the table ring) also with
    params == NULL'"""
    c = ctx()
    e = c.execute_extents((1, 2), (0, 1), MIXED2)
    assert e.status == M.OK and e.launched and e.per_frame and e.own_pass and c.ring == 1 and c.totals["per_frame"] == 1
    assert "mixed_shared_params_takes_ring_slot" in e.events
    e = c.execute_extents((1, 2), (0, 1), MIXED2, params=(P0, P1))
    assert e.per_frame and c.ring == 2 and "mixed_shared_params_takes_ring_slot" not in e.events


def test_a_mixed_call_runs_a_waiting_composite_first_as_plain_launches():
    """'a waiting composite batch is run first as plain launches' -- where a shared call of the context's size would carry it"""
    c = ctx()
    c.execute((1, 2), (0, 1), stream=1)
    c.comp_enqueue(0, (0, 1), (0, 1))
    e = c.execute_extents((3, 4), (2, 3), MIXED2)
    assert e.comp_plain == 2 and e.comp_carried == 0 and e.comp_pending == 0 and e.comp_ran.stream == 1
    assert "mixed_flushes_composite" in e.events and c.totals["comp_plain_launches"] == 2 and c.totals["comp_carried_launches"] == 0


def test_a_mixed_call_consumes_a_ready_set_unmatched_and_reports_mixed_alone():
    """'a ready prefetched set is consumed unmatched (the call runs its own downsample pass)'; the model reports "mixed" as the
    one reason, also when every component of the key would have matched, and also when none would."""
    c = ctx()
    c.prefetch((1, 2))
    c.execute((5, 6), (0, 1))
    e = c.execute_extents((1, 2), (0, 1), MIXED2)                      # the announced buffers, the same stream
    assert e.own_pass and not e.reused and e.refused == ("mixed",) and c.ready is None
    assert {"mixed_consumes_ready", "mixed_consumes_ready_same_buffers"} <= set(e.events)
    assert c.execute((1, 2), (0, 1)).refused == ()                      # gone after the one call
    c.prefetch((1, 2))
    c.execute((5, 6), (0, 1))
    e = c.execute_extents((7,), (0,), ((200, 120, 1, 2),), params=(P2,), stream=1)      # nothing of the key matches
    assert e.refused == ("mixed",) and "mixed_consumes_ready_same_buffers" not in e.events


@pytest.mark.parametrize("kind", ["plain", "pitched", "per_frame", "sized"])
def test_a_mixed_call_carries_any_announcement_as_a_launch_of_its_own_and_promotes_it(kind):
    """'an announcement (meao_prefetch_batch*, sized or not) is carried as a launch of its own behind the last kernel and promoted
    as usual': the ready set keeps the announcement's own size if sized (else the context's), its pitch, the call's stream and
    the call's exactness; its Z-buffer inputs are its own params' or the context's."""
    c = reserved()
    kw = dict(plain={}, pitched=dict(pitch=1), per_frame=dict(params=(P1, P2, P3)), sized=dict(size=(200, 120), pitch=2))[kind]
    c.prefetch((1, 2, 3), **kw)
    e = c.execute_extents((5, 6), (0, 1), MIXED2, params=(PX0, P0), stream=1)
    assert e.carried.bufs == (1, 2, 3) and e.own_pass and c.ann is None and not e.exact
    assert "mixed_carries_" + kind in e.events and "mixed_carries_more_frames_than_n" in e.events
    r = c.ready
    assert r.bufs == (1, 2, 3) and r.stream == 1 and not r.exact and r.sized == (kind == "sized")
    assert r.size == ((200, 120) if kind == "sized" else (384, 256))
    assert r.pitch == {"plain": 384, "pitched": 392, "per_frame": 384, "sized": 205}[kind]
    assert r.zb == tuple(p.zb(False) for p in ((P1, P2, P3) if kind == "per_frame" else (P0,) * 3))
    assert c.totals["carried"] == 1 and c.totals["carried_by_mixed"] == 1 and c.totals["own"] == 1
    # and the announced batch finds it: reused by an inexact call on that stream at that size, refused by an exact one
    if kind == "sized":
        assert "sized_ready_from_mixed_kept_by_resize" in c.resize(200, 120).events
    call = dict(pitch={"pitched": 1, "sized": 2}.get(kind, 0), stream=1)
    prm = (P1, P2, P3) if kind == "per_frame" else (P0, P0, P0)
    if kind != "per_frame":                     # (PX0 is P0's camera: frame 0 of the per-frame announcement has P1's)
        assert c.execute((1, 2, 3), (0, 1, 2), params=(PX0,) + prm[1:], **call).reused
    else:
        assert c.execute((1, 2, 3), (0, 1, 2), params=prm, **call).refused == ("exact",)
    c.prefetch((1, 2, 3), **{k: v for k, v in kw.items() if k != "size"})
    c.execute_extents((5, 6), (0, 1), ((33, 17, 0, 0), (97, 61, 0, 0)), stream=1)       # an exact carrier
    assert c.execute((1, 2, 3), (0, 1, 2), params=prm, **call).reused


def test_exact_of_a_mixed_call_is_every_frame_exact():
    c = ctx()
    assert c.execute_extents((1, 2), (0, 1), MIXED2).exact                               # the context's parameters for every frame
    assert not c.execute_extents((1, 2), (0, 1), MIXED2, params=(P0, PX2)).exact
    c.set_params(PX0)
    assert not c.execute_extents((1, 2), (0, 1), MIXED2).exact
    assert not ctx(rtz=False).execute_extents((1, 2), (0, 1), MIXED2).exact


def test_a_refused_mixed_call_changes_nothing():
    """'a refused call launches nothing and leaves an announcement, a ready set and a waiting composite as they were'; the
    validation order: n, params[], then each frame's size against [1, 32768] and the capacity, then each pitch against ITS frame."""
    c = reserved()
    c.prefetch((1,))
    c.execute((5,), (0,))
    c.comp_enqueue(0, (0,), (0,))
    c.prefetch((2,))
    before = (c.ann, c.ready, c.comp, c.last, c.ring, dict(c.totals))
    bad = [dict(extents=((401, 256, 0, 0),)), dict(extents=((384, 273, 0, 0),)), dict(extents=((0, 256, 0, 0),)),
           dict(extents=((384, 0, 0, 0),)), dict(extents=((32769, 1, 0, 0),)), dict(extents=((200, 120, 0, 0),), rows=((199, 200),)),
           dict(extents=((200, 120, 0, 0),), rows=((200, 199),)), dict(extents=((200, 120, 0, 0),), params=(PBAD,)),
           dict(extents=((200, 120, 0, 0),) * 5, bufs=(1, 2, 3, 4, 5)), dict(extents=(), bufs=())]
    for kw in bad:
        bufs = kw.pop("bufs", (7,))
        e = c.execute_extents(bufs, tuple(range(len(bufs))), kw.pop("extents"), **kw)
        assert e.status == M.ERR_INVALID_ARGUMENT and not e.launched and e.comp_pending == 1 and e.last_valid, kw
        assert (c.ann, c.ready, c.comp, c.last, c.ring, dict(c.totals)) == before, kw
    # a stride that is legal for its own frame although it is below the context's width, and the capacity's own size, are accepted
    assert c.execute_extents((7, 8), (1, 2), ((200, 120, 0, 0), (400, 272, 0, 0)), rows=((200, 200), (400, 408))).status == M.OK
    # without a reservation the capacity is the context's size
    c = ctx()
    assert c.execute_extents((7,), (1,), ((385, 256, 0, 0),)).status == M.ERR_INVALID_ARGUMENT
    assert c.execute_extents((7,), (1,), ((383, 256, 0, 0),)).status == M.OK


def test_uniform_extents_are_the_pitched_call():
    """'When every extent equals the context's size and all frames share their pitches the call IS meao_execute_batch_pitched':
    it reuses, carries as an ordinary call does, takes a ring slot only with per-frame constants, and lets a composite ride."""
    c = ctx()
    c.prefetch((1, 2), pitch=1)
    c.execute((5, 6), (0, 1))
    c.comp_enqueue(0, (0,), (0,))
    c.prefetch((3,))
    e = c.execute_extents((1, 2), (2, 3), ((384, 256, 1, 2),) * 2)
    assert e.reused and not e.own_pass and not e.per_frame and c.ring == 0 and e.comp_carried == 1 and e.carried.bufs == (3,)
    assert {"uniform_extents", "uniform_extents_reuses", "uniform_extents_carries"} <= set(e.events) and "mixed_call" not in e.events
    assert not c.last.mixed and c.last.depth_pitch == 392 and c.last.out_pitch == 389
    # strides are compared in texels: 0 and the packed row are one stride; two strides make the call mixed at the context's size
    assert c.extents_uniform(((384, 256, 0, 0),) * 2, rows=((384, 384), (384, 384)))
    assert not c.extents_uniform(((384, 256, 0, 0), (384, 256, 1, 0)))
    c.prefetch((1,))
    c.execute((5,), (0,))
    e = c.execute_extents((1, 2), (0, 1), ((384, 256, 0, 0), (384, 256, 0, 1)))
    assert e.refused == ("mixed",) and e.per_frame and c.last.mixed
    # with params[] it is the per-frame pitched call
    assert c.execute_extents((1,), (0,), ((384, 256, 0, 0),), params=(P1,)).per_frame


def test_last_call_of_a_mixed_call_has_per_frame_sizes_and_is_invalidated_as_ever():
    """'Afterwards meao_get_intermediate / meao_debug_view describe and return frame f's buffers at frame f's size'; a reserve, a
    resize and a re-allocation take it away as they take every last call; a refill of one of its frames makes it unreadable."""
    c = reserved()
    c.refill((1, 2), (("synth", 0), ("synth", 1)))
    e = c.execute_extents((1, 2), (0, 1), ((200, 120, 1, 0), (380, 250, 0, 2)), params=(P1, P2))
    assert c.last.mixed and c.last.n == 2 and c.last.sizes == ((200, 120), (380, 250)) and c.last.rows == ((208, 200), (380, 385))
    assert c.last.params == (P1, P2) and c.readable() and e.last_valid
    assert "mixed_then_debug_read" in c.debug_set(0, 1).events
    assert "mixed_then_debug_read" in c.invalid(M.Op("invalid", what="n_zero", on="execute")).events
    c.refill((2,), (("synth", 2),))
    assert not c.readable()
    c.execute_extents((1, 2), (0, 1), MIXED2)
    e = c.reserve(400, 272)
    assert "mixed_then_reserve_invalidates" in e.events and c.last is None and not e.last_valid
    assert "mixed_after_invalidation" in c.execute_extents((1, 2), (0, 1), MIXED2).events
    assert "mixed_then_reserve_invalidates" in c.resize(380, 250).events and c.last is None
    assert c.execute((1,), (0,)).last_valid and c.last.sizes == ((380, 250),) and not c.last.mixed
    c = ctx(pipelined=False)
    c.execute_extents((1, 2), (0, 1), MIXED2)
    assert c.prefetch((3,)).reallocated and c.last is None


def test_what_follows_a_mixed_call_obeys_the_existing_rules():
    """The ready set a mixed call leaves is an ordinary one: set_params drops it, a resize keeps a sized one for exactly its size."""
    c = reserved()
    c.prefetch((1,), size=(200, 120))
    c.execute_extents((5, 6), (0, 1), MIXED2)
    assert "sized_ready_dropped_other_size" in c.resize(380, 250).events and c.ready is None
    c.prefetch((1,), size=(200, 120))
    c.execute_extents((5, 6), (0, 1), MIXED2)
    assert "ready_dropped_by_set_params" in c.set_params(P1).events and c.ready is None
    c.prefetch((1,))
    c.execute_extents((5, 6), (0, 1), MIXED2)
    assert "unsized_dropped_by_resize_inside" in c.resize(200, 120).events


def test_a_mixed_call_on_the_other_stream_leaves_a_ready_set_of_that_stream():
    c = ctx()
    c.execute((9,), (0,), stream=0)
    c.prefetch((1,))
    e = c.execute_extents((5, 6), (0, 1), MIXED2, stream=1)
    assert "mixed_on_other_stream" in e.events and c.ready.stream == 1
    assert c.execute((1,), (0,), stream=0).refused == ("stream",)


def mixed_pool(G=3):
    return reserved_pool(G)


def test_pool_deals_extents_with_the_frames_and_each_member_classifies_its_own_share():
    """'frame f, extents[f] and params[f] (if given) go to member f mod G'; a member whose share is uniform at its size makes the
    pitched call -- it may reuse -- while the others make mixed calls and consume their ready sets unmatched."""
    p = mixed_pool()
    p.apply(M.Op("prefetch", bufs=(10, 11, 12, 13, 14, 15)))
    p.apply(M.Op("execute", bufs=(1, 2, 3, 4, 5, 6), outs=(0, 1, 2, 3, 4, 5)))
    ext = ((384, 256, 0, 0), (200, 120, 0, 0), (97, 61, 1, 0), (384, 256, 0, 0), (33, 17, 0, 2), (257, 31, 0, 0))
    e = p.apply(M.Op("execute", bufs=(10, 11, 12, 13, 14, 15), outs=(0, 1, 2, 3, 4, 5), extents=ext, params=(P0, P1, P2, P0, P4, P5)))
    assert e[0].reused and e[0].refused == () and "mixed_call" not in e[0].events
    assert all(x.own_pass and x.refused == ("mixed",) and x.per_frame for x in e[1:])
    assert {"pool_member_uniform_while_other_mixed", "pool_member_uniform_reuses_while_other_mixed"} <= set(e[0].events)
    assert p.members[1].last.sizes == ((200, 120), (33, 17)) and p.members[1].last.params == (P1, P4)
    assert p.members[2].last.rows == ((105, 97), (257, 257))


def test_pool_mixed_call_members_dealt_nothing_drop_what_they_hold():
    """'members dealt nothing do what they do for meao_pool_execute_batch_pitched': they drop announcement and ready set."""
    p = mixed_pool()
    p.apply(M.Op("prefetch", bufs=(10, 11, 12)))
    e = p.apply(M.Op("execute", bufs=(1, 2), outs=(0, 1), extents=((200, 120, 0, 0), (384, 256, 0, 0))))
    assert e[2] is None and p.members[2].ann is None and "pool_mixed_idle_member" in e[0].events
    assert e[0].carried.bufs == (10,) and "mixed_call" in e[0].events and "mixed_call" not in e[1].events and e[1].carried.bufs == (11,)
    assert "pool_member_uniform_while_other_mixed" in e[0].events


def test_pool_mixed_call_with_one_bad_share_is_refused_whole():
    """'Every member's share is validated against that member's capacity before any member enqueues'"""
    p = mixed_pool()
    p.apply(M.Op("prefetch", bufs=(10, 11, 12)))
    bad = M.Op("execute", bufs=(1, 2, 3), outs=(0, 1, 2), extents=((200, 120, 0, 0), (416, 120, 0, 0), (97, 61, 0, 0)))
    with pytest.raises(AssertionError):
        p.apply(bad)                                                    # a sequence may not hold it as a valid call
    assert p.check_extents(bad) == M.ERR_INVALID_ARGUMENT
    e = p.apply(dataclasses.replace(bad, kind="invalid", what="extent_outside_on_one_member", on="execute"))
    assert all(x.status == M.ERR_INVALID_ARGUMENT and not x.launched for x in e) and "pool_mixed_refused_whole" in e[0].events
    assert all(c.ann is not None and c.last is None for c in p.members) and p.announced_n == 3
    # n is the pool's: max_batch x members
    assert p.check_extents(M.Op("execute", bufs=tuple(range(7)), extents=((200, 120, 0, 0),) * 7)) == M.ERR_INVALID_ARGUMENT
    assert p.check_extents(M.Op("execute", bufs=tuple(range(6)), extents=((200, 120, 0, 0),) * 6)) == M.OK


def test_the_model_holds_the_generators_mixed_invalid_calls_to_the_rule_they_name():
    c = reserved()
    ok = ((200, 120, 0, 0), (97, 61, 1, 2))
    for op in (M.Op("invalid", what="extent_outside_capacity", on="execute", bufs=(1, 2), extents=ok),
               M.Op("invalid", what="extent_zero", on="execute", bufs=(1, 2), extents=((416, 120, 0, 0), (97, 61, 0, 0))),
               M.Op("invalid", what="extent_pitch_below_row", on="execute", bufs=(1, 2), extents=((0, 120, 0, 0), (97, 61, 0, 0)), value=1),
               M.Op("invalid", what="extent_bad_params", on="execute", bufs=(1, 2), extents=ok, params=(P0, P1)),
               M.Op("invalid", what="extent_n_over", on="execute", bufs=(1, 2), extents=ok)):
        with pytest.raises(AssertionError):
            c.apply(op)
    for op in (M.Op("invalid", what="extent_outside_capacity", on="execute", bufs=(1, 2), extents=((200, 120, 0, 0), (97, 280, 0, 0))),
               M.Op("invalid", what="extent_zero", on="execute", bufs=(1, 2), extents=((200, 0, 0, 0), (97, 61, 0, 0))),
               M.Op("invalid", what="extent_pitch_below_row", on="execute", bufs=(1, 2), extents=ok, key=1, value=1),
               M.Op("invalid", what="extent_bad_params", on="execute", bufs=(1, 2), extents=ok, params=(P0, PBAD)),
               M.Op("invalid", what="extent_n_over", on="execute", bufs=(1, 2, 3, 4, 5), extents=ok[:1] * 5)):
        assert c.apply(op).status == M.ERR_INVALID_ARGUMENT


def test_f32_free_running_mixed_cases_hold_carries_the_header_lets_ride():
    """The free-running tests bound the fused launches of a trace by the carried passes that include/meao.h lets ride inside an
    ordinary carrier's last kernel (M.header_lets_it_ride).  In the two f32 cases that bound must not be zero, so that the fused
    form is in play next to the mixed calls, which never use it."""
    for name in ("r8_rtz_f32", "r8_rtz_linear_f32"):
        ops, model = M.case_sequence("mix_free", name)
        assert M.may_ride_count(ops, model) >= 2, name
    ops, model = M.case_sequence("mix_free", "f16_rtne_unorm16")
    assert M.may_ride_count(ops, model, f32_depth=False) == 0          # UNORM16 depth: nothing rides
    a = M.Announcement((1, 2), 384, None, False, (384, 256))
    assert M.header_lets_it_ride(a, 2, (384, 256), True) and not M.header_lets_it_ride(a, 1, (384, 256), True)
    assert not M.header_lets_it_ride(M.Announcement((1,), 380, None, False, (380, 250)), 1, (384, 256), True)      # width % 8
    assert not M.header_lets_it_ride(M.Announcement((1,), 389, None, False, (384, 256)), 1, (384, 256), True)      # stride % 4
    assert not M.header_lets_it_ride(M.Announcement((1,), 400, None, True, (400, 272)), 1, (200, 120), True)       # tiles do not fit
    assert M.header_lets_it_ride(M.Announcement((1,), 200, None, True, (200, 120)), 1, (384, 256), True)
