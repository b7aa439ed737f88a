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
