"""Several cameras per batch: what per-frame parameters cost, at 4K, S2 frames, 16 frames per step, HIP events.

    python tools/frame_params_rate.py [--rounds 5] [--steps 60] [--out profiles/frame_params_rate.jsonl]

Three arms, alternated round by round in one process (each >= 100 ms in total):
  shared     meao_execute_batch, one camera, pipelined (meao_prefetch_batch)
  per_frame  meao_execute_batch_params, 16 distinct cameras, pipelined (meao_prefetch_batch_params)
  set_params 16 calls of one frame each with meao_set_params between them (mixing cameras without this API)
One JSON line per arm and round, then a summary line (medians, per_frame / shared, set_params / per_frame).
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

from miniengineao_amd import AmbientOcclusion, FrameParams, synth  # noqa: E402
from miniengineao_amd import _lib as L  # noqa: E402
from miniengineao_amd.frame_params import params_array  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    w, h, B = 3840, 2160, 16
    cam = synth.DEFAULT_CAMERA
    dev = torch.device("cuda", 0)
    sets = [[torch.from_numpy(synth.make("S2", w, h, seed=0x1234ABCD + 16 * k + f)).to(dev) for f in range(B)] for k in range(2)]
    outs = [torch.empty((h, w), dtype=torch.uint8, device=dev) for _ in range(B)]
    ao = AmbientOcclusion(w, h, max_batch=B, pipelined=True, near_clip=cam.near, far_clip=cam.far, projection00=cam.proj00(w, h))
    lib, ctx = ao._lib, ao._ctx
    ao.execute_device([t.data_ptr() for t in sets[0]], [t.data_ptr() for t in outs])        # parameters applied, warm
    torch.cuda.synchronize(dev)
    stream = torch.cuda.Stream(dev)          # a stream of its own: the events and every launch of the three arms are on it
    st = C.c_void_p(stream.cuda_stream)
    rng = np.random.default_rng(16)
    cams = [FrameParams(nearClipPlane=float(np.float32(rng.uniform(0.05, 0.5))), farClipPlane=float(np.float32(rng.uniform(50, 5000))),
                        projection00=synth.Camera(fov_y_deg=float(rng.uniform(30, 90))).proj00(w, h)) for _ in range(B)]
    prm = params_array(cams, B, ao._prm)
    single = [(L.Params * 1)(prm[f]) for f in range(B)]
    pin = [(C.c_void_p * B)(*[t.data_ptr() for t in s]) for s in sets]
    pout = (C.c_void_p * B)(*[t.data_ptr() for t in outs])
    one_in = [[(C.c_void_p * 1)(t.data_ptr()) for t in s] for s in sets]
    one_out = [(C.c_void_p * 1)(t.data_ptr()) for t in outs]

    def shared(k):
        L.check(lib.meao_prefetch_batch(ctx, B, pin[(k + 1) & 1]), ctx)
        L.check(lib.meao_execute_batch(ctx, B, pin[k & 1], L.MEM_DEVICE, pout, L.MEM_DEVICE, st), ctx)

    def per_frame(k):
        L.check(lib.meao_prefetch_batch_params(ctx, B, pin[(k + 1) & 1], prm), ctx)
        L.check(lib.meao_execute_batch_params(ctx, B, pin[k & 1], L.MEM_DEVICE, pout, L.MEM_DEVICE, prm, st), ctx)

    def set_params(k):
        for f in range(B):
            L.check(lib.meao_set_params(ctx, single[f]), ctx)
            L.check(lib.meao_execute_batch(ctx, 1, one_in[k & 1][f], L.MEM_DEVICE, one_out[f], L.MEM_DEVICE, st), ctx)

    arms = {"shared": shared, "per_frame": per_frame, "set_params": set_params}
    res = {k: [] for k in arms}
    lines = []
    for name, fn in arms.items():          # warm-up of every arm
        for k in range(3):
            fn(k)
    L.check(lib.meao_set_params(ctx, C.byref(ao._prm)), ctx)
    torch.cuda.synchronize(dev)
    for r in range(a.rounds):
        for name, fn in arms.items():
            if name == "shared":
                L.check(lib.meao_set_params(ctx, C.byref(ao._prm)), ctx)
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
    med = {k: statistics.median(v) for k, v in res.items()}
    summary = {"summary": True, "width": w, "height": h, "frames_per_step": B,
               "median_us_per_frame": {k: round(v, 3) for k, v in med.items()},
               "ms_per_arm": {k: round(sum(v) * a.steps * B / 1e3, 1) for k, v in res.items()},
               "per_frame_over_shared": round(med["per_frame"] / med["shared"], 4),
               "set_params_over_per_frame": round(med["set_params"] / med["per_frame"], 3),
               "device": torch.cuda.get_device_name(dev)}
    print(json.dumps(summary), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            for ln in lines + [summary]:
                fh.write(json.dumps(ln) + "\n")
    ao.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
