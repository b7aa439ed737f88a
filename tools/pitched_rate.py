"""Row-pitched surfaces: what reading depth and writing AO in place inside larger surfaces costs, at 4K, S2 frames, 16 frames per
step, pipelined, HIP events.

    python tools/pitched_rate.py [--rounds 5] [--steps 60] [--out profiles/pitched_rate.jsonl]

Three arms, alternated round by round in one process (each >= 100 ms in total):
  packed     meao_execute_batch + meao_prefetch_batch on tightly packed frames
  aligned    meao_execute_batch_pitched + meao_prefetch_batch_pitched, rows of 4096 texels (a 256-byte multiple: the vector forms)
  unaligned  the same with rows of 3841 texels (not a multiple of 4 texels: the scalar forms, the next pass as its own launch)
One JSON line per arm and round, then a summary line (medians, aligned / packed, unaligned / packed).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from miniengineao_amd import AmbientOcclusion, synth  # noqa: E402
from miniengineao_amd import _lib as L  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    w, h, B = 3840, 2160, 16
    cam = synth.DEFAULT_CAMERA
    dev = torch.device("cuda", 0)
    frames = [[torch.from_numpy(synth.make("S2", w, h, seed=0x1234ABCD + 16 * k + f)) for f in range(B)] for k in range(2)]
    pitches = {"packed": w, "aligned": 4096, "unaligned": 3841}
    surf, outs = {}, {}
    for name, p in pitches.items():        # frame f of set k at the top-left of a (h, p) surface; the padding stays NaN
        surf[name] = []
        for k in range(2):
            s = torch.full((B, h, p), float("nan"), dtype=torch.float32, device=dev)
            for f in range(B):
                s[f, :, :w] = frames[k][f].to(dev)
            surf[name].append(s)
        outs[name] = torch.zeros((B, h, p), dtype=torch.uint8, device=dev)
    ao = AmbientOcclusion(w, h, max_batch=B, pipelined=True, near_clip=cam.near, far_clip=cam.far, projection00=cam.proj00(w, h))
    lib, ctx = ao._lib, ao._ctx
    torch.cuda.synchronize(dev)
    stream = torch.cuda.Stream(dev)
    st = C.c_void_p(stream.cuda_stream)
    P = C.c_void_p * B
    pin = {n: [P(*[s[f].data_ptr() for f in range(B)]) for s in surf[n]] for n in pitches}
    pout = {n: P(*[outs[n][f].data_ptr() for f in range(B)]) for n in pitches}

    def arm(name):
        dp, op = pitches[name] * 4, pitches[name]

        def step(k):
            if name == "packed":
                L.check(lib.meao_prefetch_batch(ctx, B, pin[name][(k + 1) & 1]), ctx)
                L.check(lib.meao_execute_batch(ctx, B, pin[name][k & 1], L.MEM_DEVICE, pout[name], L.MEM_DEVICE, st), ctx)
            else:
                L.check(lib.meao_prefetch_batch_pitched(ctx, B, pin[name][(k + 1) & 1], dp, None), ctx)
                L.check(lib.meao_execute_batch_pitched(ctx, B, pin[name][k & 1], dp, L.MEM_DEVICE, pout[name], op, L.MEM_DEVICE,
                                                       None, st), ctx)
        return step

    arms = {n: arm(n) for n in pitches}
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
            lines.append({"arm": name, "pitch_texels": pitches[name], "round": r, "steps": a.steps, "frames_per_step": B,
                          "ms": round(ms, 3), "us_per_frame": round(us_frame, 3)})
            print(json.dumps(lines[-1]), flush=True)
    torch.cuda.synchronize(dev)
    same = all(torch.equal(outs["packed"], outs[n][:, :, :w]) for n in ("aligned", "unaligned"))
    med = {k: statistics.median(v) for k, v in res.items()}
    summary = {"summary": True, "width": w, "height": h, "frames_per_step": B,
               "median_us_per_frame": {k: round(v, 3) for k, v in med.items()},
               "ms_per_arm": {k: round(sum(v) * a.steps * B / 1e3, 1) for k, v in res.items()},
               "aligned_over_packed": round(med["aligned"] / med["packed"], 4),
               "unaligned_over_packed": round(med["unaligned"] / med["packed"], 4),
               "results_identical": same, "device": torch.cuda.get_device_name(dev)}
    print(json.dumps(summary), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            for ln in lines + [summary]:
                fh.write(json.dumps(ln) + "\n")
    ao.close()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
