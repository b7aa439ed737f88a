"""The call-sequence model (tests/call_model.py, unchanged) against a context that holds a reservation.

The model only ever emits the existing calls, whose observable rules do not change under a reservation: a resize still drops every
announcement and ready set those calls made, still runs a waiting composite at the old size, still invalidates the debug state.  The
sequences here draw their resizes from three sizes, and the context is given a reservation that covers all three before the first
operation -- so every resize of the sequence is one that moves no buffer.  The driver is that of tests/test_call_sequences_gpu.py:
it builds its context in its constructor, and the reservation is made on that context before the sequence runs."""
import pytest

from tests import call_model as M
from tests import test_call_sequences_gpu as S

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
        d.run(ops, model)
        assert d.ao.capacity == (wmax, hmax)            # no resize of the sequence left the reservation
    finally:
        d.close()
