"""Linear view-space depth input: what reading z instead of a hardware depth buffer costs, at 4K, S2 frames, 16 frames per step,
pipelined (the fused last kernel carries the next batch's downsample pass), HIP events.

    python tools/linear_depth_rate.py [--rounds 5] [--steps 60] [--out profiles/linear_depth_rate.jsonl]

Three arms, one context each, alternated round by round in one process (each >= 100 ms in total):
  raw_f32     MEAO_DEPTH_F32: the hardware depth of the S2 frames (camera far_clip = 128)
  linear_f32  MEAO_DEPTH_LINEAR_F32: z = Linearize(depth) * far of the same frames
  linear_f16  MEAO_DEPTH_LINEAR_F16: the same z as float16 (half the bytes in both depth-reading passes)
One JSON line per arm and round, then a summary line (medians, linear / raw).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from miniengineao_amd import AmbientOcclusion, synth  # noqa: E402
from miniengineao_amd import _lib as L  # noqa: E402


def linear_z(d, cam):
    """Linear view-space z of raw reversed-Z depth d (f64 arithmetic: a timing input, not a parity reference)."""
    fpn = float(np.float32(cam.far) / np.float32(cam.near))
    with np.errstate(divide="ignore"):
        dist = 1.0 / ((fpn - 1.0) * d.astype(np.float64) + 1.0)
    dist[d == 0] = 1.0
    return (dist * cam.far).astype(np.float32)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    w, h, B = 3840, 2160, 16
    cam = synth.Camera(near=0.1, far=128.0, reversed_z=True)
    dev = torch.device("cuda", 0)
    raw = [[synth.occluder_field(w, h, seed=0x1234ABCD + 16 * k + f, cam=cam) for f in range(B)] for k in range(2)]
    fmts = {"raw_f32": L.DEPTH_F32, "linear_f32": L.DEPTH_LINEAR_F32, "linear_f16": L.DEPTH_LINEAR_F16}
    sets = {"raw_f32": [torch.from_numpy(np.stack(s)).to(dev) for s in raw]}
    sets["linear_f32"] = [torch.from_numpy(np.stack([linear_z(d, cam) for d in s])).to(dev) for s in raw]
    sets["linear_f16"] = [t.half() for t in sets["linear_f32"]]
    outs = {n: torch.zeros((B, h, w), dtype=torch.uint8, device=dev) for n in fmts}
    ctxs = {n: AmbientOcclusion(w, h, max_batch=B, pipelined=True, near_clip=cam.near, far_clip=cam.far, projection00=cam.proj00(w, h),
                                depth_format=f) for n, f in fmts.items()}
    torch.cuda.synchronize(dev)
    stream = torch.cuda.Stream(dev)
    st = C.c_void_p(stream.cuda_stream)
    P = C.c_void_p * B
    pin = {n: [P(*[s[f].data_ptr() for f in range(B)]) for s in sets[n]] for n in fmts}
    pout = {n: P(*[outs[n][f].data_ptr() for f in range(B)]) for n in fmts}

    def arm(name):
        lib, ctx = ctxs[name]._lib, ctxs[name]._ctx

        def step(k):
            L.check(lib.meao_prefetch_batch(ctx, B, pin[name][(k + 1) & 1]), ctx)
            L.check(lib.meao_execute_batch(ctx, B, pin[name][k & 1], L.MEM_DEVICE, pout[name], L.MEM_DEVICE, st), ctx)
        return step

    arms = {n: arm(n) for n in fmts}
    res = {k: [] for k in arms}
    lines = []
    for fn in arms.values():               # warm-up of every arm
        for k in range(3):
            fn(k)
    torch.cuda.synchronize(dev)
    for r in range(a.rounds):
        for name, fn in arms.items():
            fn(0)                          # the first step of an arm primes its prefetch
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for k in range(1, a.steps + 1):
                fn(k)
            e1.record(stream)
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            us_frame = ms * 1e3 / (a.steps * B)
            res[name].append(us_frame)
            lines.append({"arm": name, "round": r, "steps": a.steps, "frames_per_step": B, "ms": round(ms, 3),
                          "us_per_frame": round(us_frame, 3)})
            print(json.dumps(lines[-1]), flush=True)
    torch.cuda.synchronize(dev)
    med = {k: statistics.median(v) for k, v in res.items()}
    summary = {"summary": True, "width": w, "height": h, "frames_per_step": B,
               "median_us_per_frame": {k: round(v, 3) for k, v in med.items()},
               "range_us_per_frame": {k: [round(min(v), 3), round(max(v), 3)] for k, v in res.items()},
               "ms_per_arm": {k: round(sum(v) * a.steps * B / 1e3, 1) for k, v in res.items()},
               "linear_f32_over_raw_f32": round(med["linear_f32"] / med["raw_f32"], 4),
               "linear_f16_over_raw_f32": round(med["linear_f16"] / med["raw_f32"], 4),
               "device": torch.cuda.get_device_name(dev)}
    print(json.dumps(summary), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            for ln in lines + [summary]:
                fh.write(json.dumps(ln) + "\n")
    for c in ctxs.values():
        c.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
