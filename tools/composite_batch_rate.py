"""The batched composite against per-frame launches: color.rgba *= ao (MULTIPLY) of a whole batch of tightly packed frames with
R8 AO, as n meao_composite_format launches and as one meao_composite_batch launch.  HIP events around `steps` passes over the batch.

    python tools/composite_batch_rate.py [--rounds 5] [--steps 20] [--out profiles/composite_batch_rate.jsonl] [--skip-shaded]

Shapes: 3840 x 2160 x 16 RGBA16F, 1920 x 1080 x 64 RGBA8, 640 x 360 x 64 R11G11B10F.  The two arms of a shape are alternated round
by round in one process, the colours reset before every timed round; the first frame of each arm is checked against the NumPy
model of tests/color_formats.py after one pass (the tool runs from a checkout: it imports the model from the tests package).  One
JSON line per arm and round, then a summary line per shape: median, slowest and fastest round of each arm in Gpixels/s, and the
ratio of the medians (batched over per-frame).

Then, at 3840 x 2160 x 16 RGBA16F, AO plus shaded frames per step three ways: meao_execute_batch + 16 meao_composite launches,
meao_execute_batch_shaded, and the carried form (meao_composite_enqueue; the next step's render kernel composites this step's
frames).  Reported only.
"""
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
from tools.composite_format_rate import initial, model  # noqa: E402

SHAPES = [(3840, 2160, 16, "RGBA16F", L.COLOR_RGBA16F), (1920, 1080, 64, "RGBA8", L.COLOR_RGBA8),
          (640, 360, 64, "R11G11B10F", L.COLOR_R11G11B10F)]


def timed(stream, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def composite_shape(a, dev, w, h, B, name, fmt, lines):
    aosurf = torch.randint(0, 256, (B, h, w), device=dev, dtype=torch.uint8)
    color0 = initial(fmt, B, h, w, dev)
    color = torch.empty_like(color0)
    ao = AmbientOcclusion(w, h, max_batch=B)
    stream = torch.cuda.Stream(dev)
    st = stream.cuda_stream
    aptr, cptr = [aosurf[f].data_ptr() for f in range(B)], [color[f].data_ptr() for f in range(B)]

    def per_frame(count):
        for _ in range(count):
            for f in range(B):
                ao.composite_device(L.COMPOSITE_MULTIPLY, aptr[f], cptr[f], 0, st, color_format=fmt)

    def batched(count):
        for _ in range(count):
            ao.composite_batch_device(L.COMPOSITE_MULTIPLY, aptr, cptr, None, st, color_format=fmt)

    arms = {"per_frame_launches": per_frame, "one_batched_launch": batched}
    ok = True
    want = model(fmt, aosurf[0].cpu().numpy(), color0[0].cpu().numpy())
    for arm, fn in arms.items():                                 # one pass, checked
        color.copy_(color0)
        torch.cuda.synchronize(dev)
        fn(1)
        stream.synchronize()
        got = color[0].cpu().numpy()
        same = np.array_equal(got.view(np.uint8).reshape(-1), np.ascontiguousarray(want).view(np.uint8).reshape(-1))
        print(json.dumps({"shape": [w, h, B], "format": name, "arm": arm, "first_frame_equals_the_model": bool(same)}), flush=True)
        ok = ok and same
    res = {k: [] for k in arms}
    for r in range(-1, a.rounds):                                # round -1: warm-up
        for arm, fn in arms.items():
            color.copy_(color0)
            torch.cuda.synchronize(dev)
            ms = timed(stream, lambda: fn(a.steps))
            if r < 0:
                continue
            gpix = w * h * B * a.steps / ms / 1e6
            res[arm].append(gpix)
            lines.append({"shape": [w, h, B], "format": name, "arm": arm, "round": r, "steps": a.steps, "ms": round(ms, 3),
                          "us_per_step": round(ms * 1e3 / a.steps, 2), "Gpixels_per_s": round(gpix, 2)})
            print(json.dumps(lines[-1]), flush=True)
    med = {k: statistics.median(v) for k, v in res.items()}
    lo, hi = min(res["per_frame_launches"]), max(res["per_frame_launches"])
    summary = {"summary": True, "shape": [w, h, B], "format": name, "ao_format": "R8", "mode": "MULTIPLY",
               "median_Gpixels_per_s": {k: round(v, 2) for k, v in med.items()},
               "min_max_Gpixels_per_s": {k: [round(min(v), 2), round(max(v), 2)] for k, v in res.items()},
               "batched_over_per_frame": round(med["one_batched_launch"] / med["per_frame_launches"], 4),
               "batched_median_vs_per_frame_range": "above" if med["one_batched_launch"] > hi else "inside" if med["one_batched_launch"] >= lo else "below",
               "results_equal_the_model": ok, "device": torch.cuda.get_device_name(dev)}
    lines.append(summary)
    print(json.dumps(summary), flush=True)
    ao.close()
    return ok


def shaded(a, dev, lines):
    w, h, B = 3840, 2160, 16
    depth = torch.from_numpy(synth.make("S2", w, h, seed=3)).to(dev).unsqueeze(0).repeat(B, 1, 1).contiguous()
    out = torch.zeros((B, h, w), dtype=torch.uint8, device=dev)
    color0 = initial(L.COLOR_RGBA16F, B, h, w, dev)
    color = torch.empty_like(color0)
    ao = AmbientOcclusion(w, h, max_batch=B)
    stream = torch.cuda.Stream(dev)
    st = stream.cuda_stream
    dptr, optr, cptr = ([t[f].data_ptr() for f in range(B)] for t in (depth, out, color))
    M = L.COMPOSITE_MULTIPLY

    def launches(count):
        for _ in range(count):
            ao.execute_device(dptr, optr, st)
            for f in range(B):
                ao.composite_device(M, optr[f], cptr[f], 0, st)

    def one_call(count):
        for _ in range(count):
            ao.execute_shaded_device(dptr, optr, M, cptr, None, st)

    def carried(count):                                          # step k's frames are composited inside step k + 1's render kernel
        for _ in range(count):
            ao.execute_device(dptr, optr, st)
            ao.composite_enqueue_device(M, optr, cptr)
        ao.composite_flush(st)

    arms = {"execute_plus_16_launches": launches, "execute_batch_shaded": one_call, "carried_by_next_render": carried}
    res = {k: [] for k in arms}
    for r in range(-1, a.rounds):
        for arm, fn in arms.items():
            color.copy_(color0)
            torch.cuda.synchronize(dev)
            ms = timed(stream, lambda: fn(a.steps))
            if r < 0:
                continue
            gpix = w * h * B * a.steps / ms / 1e6
            res[arm].append(gpix)
            lines.append({"shaded": True, "shape": [w, h, B], "format": "RGBA16F", "arm": arm, "round": r, "steps": a.steps,
                          "ms": round(ms, 3), "us_per_step": round(ms * 1e3 / a.steps, 2), "Gpixels_per_s": round(gpix, 2)})
            print(json.dumps(lines[-1]), flush=True)
    summary = {"summary": True, "shaded": True, "shape": [w, h, B], "format": "RGBA16F",
               "median_Gpixels_per_s": {k: round(statistics.median(v), 2) for k, v in res.items()},
               "min_max_Gpixels_per_s": {k: [round(min(v), 2), round(max(v), 2)] for k, v in res.items()},
               "device": torch.cuda.get_device_name(dev)}
    lines.append(summary)
    print(json.dumps(summary), flush=True)
    ao.close()


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-shaded", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines, ok = [], True
    for w, h, B, name, fmt in SHAPES:
        ok = composite_shape(a, dev, w, h, B, name, fmt, lines) and ok
        torch.cuda.empty_cache()
    if not a.skip_shaded:
        shaded(a, dev, lines)
    if a.out:
        with open(a.out, "w") as fh:
            for ln in lines:
                fh.write(json.dumps(ln) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
