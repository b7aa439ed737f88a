"""Shaded frames from mixed-size batches: AO plus color.rgba *= ao (MULTIPLY) of a batch of frames of several sizes, R8 AO, tightly
packed surfaces, on a 3840 x 2160 context with max_batch 16 and a reservation of its own size.  HIP events around `steps` passes.

    python tools/mixed_shaded_rate.py [--rounds 5] [--steps 10] [--out profiles/mixed_shaded_rate.jsonl] [--skip-kernel]

Batches: one 3840 x 2160 frame plus fifteen 256 x 256 frames ("main_plus_probes"), and sixteen frames of four sizes from
640 x 360 to 1920 x 1080 ("four_sizes"); colour in RGBA16F and RGBA8.  Arms, alternated round by round in one process with the
colours reset before every timed round:

  resize_per_group   what a host did before meao_execute_batch_extents_shaded: meao_execute_batch_extents, then per size group one
                     meao_resize inside the reservation plus one meao_composite_batch
  one_shaded_call    meao_execute_batch_extents_shaded

The first frame of each arm is checked after one pass: its colour against the NumPy model of tests/color_formats.py applied to the AO
the call wrote (the tool runs from a checkout: it imports the model from the tests package).

Then the kernel alone at 3840 x 2160 x 16 packed RGBA16F: meao_composite_batch (the packed 1-D form) against
meao_composite_batch_extents given sixteen equal extents with two different colour strides (frame 15 lies in a surface 8 texels
wider), which makes it the sized launch: every frame in the row form.  That is the cost of the row form on large packed frames.

One JSON line per arm and round, then a summary line per batch and format: median, slowest and fastest round of each arm in
microseconds per step.  Reported only; no ratio is asserted."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from miniengineao_amd import AmbientOcclusion  # noqa: E402
from miniengineao_amd import _lib as L  # noqa: E402
from miniengineao_amd import synth  # noqa: E402
from tools.composite_batch_rate import timed  # noqa: E402
from tools.composite_format_rate import initial, model  # noqa: E402

CTX = (3840, 2160)
BATCHES = {"main_plus_probes": [CTX] + [(256, 256)] * 15,
           "four_sizes": [(640, 360)] * 4 + [(960, 540)] * 4 + [(1280, 720)] * 4 + [(1920, 1080)] * 4}
FORMATS = [("RGBA16F", L.COLOR_RGBA16F), ("RGBA8", L.COLOR_RGBA8)]
M = L.COMPOSITE_MULTIPLY


def summarise(lines, res, **what):
    summary = {"summary": True, **what,
               "median_us_per_step": {k: round(statistics.median(v), 2) for k, v in res.items()},
               "min_max_us_per_step": {k: [round(min(v), 2), round(max(v), 2)] for k, v in res.items()},
               "device": torch.cuda.get_device_name(0)}
    lines.append(summary)
    print(json.dumps(summary), flush=True)


def run_arms(a, dev, stream, arms, reset, lines, **what):
    res = {k: [] for k in arms}
    for r in range(-1, a.rounds):                                # round -1: warm-up
        for arm, fn in arms.items():
            reset()
            torch.cuda.synchronize(dev)
            ms = timed(stream, lambda: fn(a.steps))
            if r < 0:
                continue
            res[arm].append(ms * 1e3 / a.steps)
            lines.append({**what, "arm": arm, "round": r, "steps": a.steps, "ms": round(ms, 3), "us_per_step": round(ms * 1e3 / a.steps, 2)})
            print(json.dumps(lines[-1]), flush=True)
    summarise(lines, res, **what)


def mixed(a, dev, ao, name, sizes, fmt_name, fmt, lines):
    n = len(sizes)
    depth = [torch.from_numpy(synth.make("S2", w, h, seed=3 + f)).to(dev) for f, (w, h) in enumerate(sizes)]
    out = [torch.zeros((h, w), dtype=torch.uint8, device=dev) for w, h in sizes]
    color0 = [initial(fmt, 1, h, w, dev)[0] for w, h in sizes]
    color = [torch.empty_like(c) for c in color0]
    stream = torch.cuda.Stream(dev)
    st = stream.cuda_stream
    dptr, optr, cptr = ([t.data_ptr() for t in ts] for ts in (depth, out, color))
    extents = [(w, h) for w, h in sizes]
    groups = {}
    for f, s in enumerate(sizes):
        groups.setdefault(s, []).append(f)

    def resize_per_group(count):
        for _ in range(count):
            ao.execute_device(dptr, optr, st, extents=extents)
            for (w, h), fs in groups.items():
                ao.resize(w, h)
                ao.composite_batch_device(M, [optr[f] for f in fs], [cptr[f] for f in fs], None, st, color_format=fmt)

    def one_shaded_call(count):
        for _ in range(count):
            ao.execute_shaded_device(dptr, optr, M, cptr, None, st, color_format=fmt, extents=extents)

    def reset():
        for c, c0 in zip(color, color0):
            c.copy_(c0)

    arms = {"resize_per_group": resize_per_group, "one_shaded_call": one_shaded_call}
    what = dict(batch=name, frames=n, format=fmt_name)
    ok = True
    for arm, fn in arms.items():                                 # one pass, checked
        reset()
        torch.cuda.synchronize(dev)
        fn(1)
        stream.synchronize()
        want = model(fmt, out[0].cpu().numpy(), color0[0].cpu().numpy())
        same = np.array_equal(color[0].cpu().numpy().view(np.uint8).reshape(-1), np.ascontiguousarray(want).view(np.uint8).reshape(-1))
        print(json.dumps({**what, "arm": arm, "first_frame_equals_the_model": bool(same)}), flush=True)
        ok = ok and same
    run_arms(a, dev, stream, arms, reset, lines, **what)
    ao.resize(*CTX)
    return ok


def kernel_alone(a, dev, ao, lines):
    w, h = CTX
    B = 16
    aosurf = torch.randint(0, 256, (B, h, w), device=dev, dtype=torch.uint8)
    color0 = initial(L.COLOR_RGBA16F, B, h, w, dev)
    color = torch.empty_like(color0)
    wide = torch.empty((h, w + 8, 4), dtype=color0.dtype, device=dev)     # frame 15 of the sized arm: another colour stride
    stream = torch.cuda.Stream(dev)
    st = stream.cuda_stream
    aptr, cptr = [aosurf[f].data_ptr() for f in range(B)], [color[f].data_ptr() for f in range(B)]
    cptr_two = cptr[:B - 1] + [wide.data_ptr()]
    extents = [(w, h, 0, 0, 0)] * (B - 1) + [(w, h, 0, (w + 8) * 8, 0)]

    def packed_1d(count):
        for _ in range(count):
            ao.composite_batch_device(M, aptr, cptr, None, st)

    def sized_rows(count):
        for _ in range(count):
            ao.composite_batch_device(M, aptr, cptr_two, None, st, extents=extents)

    def reset():
        color.copy_(color0)
        wide[:, :w].copy_(color0[B - 1])

    arms = {"composite_batch_packed_1d": packed_1d, "composite_batch_extents_rows": sized_rows}
    what = dict(kernel_alone=True, shape=[w, h, B], format="RGBA16F")
    ok = True
    want = model(L.COLOR_RGBA16F, aosurf[0].cpu().numpy(), color0[0].cpu().numpy())
    for arm, fn in arms.items():
        reset()
        torch.cuda.synchronize(dev)
        fn(1)
        stream.synchronize()
        same = np.array_equal(color[0].cpu().numpy().view(np.uint16), want)
        print(json.dumps({**what, "arm": arm, "first_frame_equals_the_model": bool(same)}), flush=True)
        ok = ok and same
    run_arms(a, dev, stream, arms, reset, lines, **what)
    return ok


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-kernel", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    ao = AmbientOcclusion(*CTX, max_batch=16)
    ao.reserve(*CTX)
    lines, ok = [], True
    for name, sizes in BATCHES.items():
        for fmt_name, fmt in FORMATS:
            ok = mixed(a, dev, ao, name, sizes, fmt_name, fmt, lines) and ok
            torch.cuda.empty_cache()
    if not a.skip_kernel:
        ok = kernel_alone(a, dev, ao, lines) and ok
    ao.close()
    if a.out:
        with open(a.out, "w") as fh:
            for ln in lines:
                fh.write(json.dumps(ln) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
