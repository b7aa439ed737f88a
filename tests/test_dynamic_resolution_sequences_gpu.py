"""The call-sequence model (tests/call_model.py) against contexts and pools that hold a reservation.

Two kinds of sequence.  The first three cases are older than the model's dynamic-resolution rules and stay as they were (their
operations are pinned by digest in tests/test_call_model.py): they draw only the calls that existed before meao_reserve, whose
observable rules do not change under a reservation -- a resize still drops every announcement and ready set those calls made, still
runs a waiting composite at the old size, still invalidates the debug state -- and the context is given a reservation that covers
all three sizes before the first operation, so every resize of the sequence is one that moves no buffer.

The others (M.dynamic_sequences) draw the rules themselves, in combination with everything else the model knows: meao_reserve in
mid-sequence (the same again, larger, (0, 0), one below the current size), resizes inside the reservation and to a size outside it
that is wider but shorter (the reservation must become 416 x 272), sized announcements -- pitched, per-frame, of more frames than
their carrier, the first announcement of a context created without cfg.pipelined -- that a resize keeps, as an announcement or as
the ready set it became, for exactly the new size and drops otherwise, with a composite waiting across the resize, an invalid
call, meao_set_params or another reserve in between; and the pool's forms of all of it, members sitting calls out included.  The
free-running cases resize inside the reservation without ever waiting.  The driver is that of tests/test_call_sequences_gpu.py; after
every reserve and resize (and every refused one) it compares every member's size and capacity with the model's."""
import pytest

from tests import call_model as M
from tests import test_call_sequences_gpu as S          # the call-sequence driver stays in its suite

pytestmark = pytest.mark.gpu

SIZES = ((384, 256), (380, 250), (200, 120))
PROFILE = M.Profile(sizes=SIZES, w_resize=4.0, p_ann_disturbed=0.35)
CASES = {"r8_rtz_f32": dict(seed=8126), "f16_rtne_unorm16": dict(seed=8126, ao="f16", rtz=False, depth="unorm16"),
         "r8_rtz_hq2": dict(seed=8127, hq_levels=2)}


def sequence(cfg):
    linear, rtz, pipelined = cfg.get("linear", False), cfg.get("rtz", True), cfg.get("pipelined", True)
    pal = M.palette(linear)
    ops = M.generate(cfg["seed"], PROFILE, pal, pal[0], linear=linear, rtz=rtz, pipelined=pipelined)
    kw = dict(linear=linear, rtz=rtz, pipelined=pipelined)
    return ops, M.ContextModel(*SIZES[0], PROFILE.max_batch, pal[0], **kw)


def test_the_sequences_resize_between_all_three_sizes():
    """(no GPU work) every case resizes several times and reaches each of the three sizes"""
    for name, cfg in CASES.items():
        ops, _ = sequence(cfg)
        sizes = [op.size for op in ops if op.kind == "resize"]
        assert len(sizes) >= 4 and set(sizes) == set(SIZES), (name, sizes)


@pytest.mark.parametrize("own_launch", [0, 1])
@pytest.mark.parametrize("name", sorted(CASES))
def test_stepped_sequence_under_a_reservation(oracle, name, own_launch):
    ops, model = sequence(CASES[name])
    wmax, hmax = max(s[0] for s in SIZES), max(s[1] for s in SIZES)
    d = S.Driver(oracle, CASES[name], PROFILE, own_launch, None, stepped=True, seed=CASES[name]["seed"])
    try:
        d.ao.reserve(wmax, hmax)
        assert d.ao.capacity == (wmax, hmax)
        model.cap = (wmax, hmax)                        # (the model's resize decides by it; these sequences hold nothing it keeps)
        d.run(ops, model)
        assert d.ao.capacity == (wmax, hmax)            # no resize of the sequence left the reservation
    finally:
        d.close()


# ---- sequences that draw reservations, resizes and sized announcements

def run_stepped(oracle, lin_c, kind, name, own_launch):
    ops, model = M.case_sequence(kind, name)
    cfg, prof, seed = M.case_profile(kind, name)
    d = S.Driver(oracle, cfg, prof, own_launch, lin_c, stepped=True, seed=seed)
    try:
        d.run(ops, model)
    finally:
        d.close()


@pytest.fixture(scope="module")
def lin_c():
    from tests.linear_depth import linearize
    return linearize()


@pytest.mark.parametrize("own_launch", [0, 1])
@pytest.mark.parametrize("name", sorted(M.DYN_CASES))
def test_stepped_sequence_with_reservations_and_sized_announcements(oracle, lin_c, name, own_launch):
    run_stepped(oracle, lin_c, "dyn_stepped", name, own_launch)


@pytest.mark.parametrize("own_launch", [0, 1])
@pytest.mark.parametrize("name", sorted(M.DYN_POOL_CASES))
def test_pool_stepped_sequence_with_resizes_and_sized_announcements(oracle, name, own_launch):
    run_stepped(oracle, None, "dyn_pool_stepped", name, own_launch)


@pytest.mark.parametrize("own_launch", [0, 1])
@pytest.mark.parametrize("name", sorted(M.DYN_FREE_CASES))
def test_free_running_sequence_with_resizes_and_sized_announcements(tmp_path, name, own_launch):
    """Nothing in it waits: the context is reserved before the first operation, every resize stays inside the reservation.  The
    trace invariants of run_free hold whatever the tile fit of a sized carried pass decides (inside the last kernel or behind it)."""
    standalone, fused, model = S.run_free(tmp_path, "dyn_free", name, own_launch)
    assert model["kept_by_resize"] >= 4 and model["carried_sized"] >= 2, model


@pytest.mark.parametrize("own_launch", [0, 1])
@pytest.mark.parametrize("name", sorted(M.DYN_POOL_CASES))
def test_pool_free_running_sequence_with_resizes_and_sized_announcements(tmp_path, name, own_launch):
    standalone, fused, model = S.run_free(tmp_path, "dyn_pool_free", name, own_launch)
    assert model["kept_by_resize"] >= 4 and model["carried_sized"] >= 2, model
