"""The composite into row-pitched surfaces against the packed one: the "depth in -> shaded frame out" step of bench.py --shaded (AO of
16 frames at 4K + color.rgba *= ao of those frames), once with tightly packed AO / RGBA16F surfaces and once with surfaces whose
pitch is one 16-byte step larger than the packed row.  HIP events, S2 frames.

    python tools/composite_pitched_rate.py [--rounds 5] [--steps 20] [--out profiles/composite_pitched_rate.jsonl]

Four arms, alternated round by round in one process:
  packed_carried    meao_composite_enqueue: the composite rides inside the next step's render kernel
  pitched_carried   meao_composite_enqueue_pitched, the same
  packed_separate   meao_composite per frame after the step's execute
  pitched_separate  meao_composite_pitched per frame
One JSON line per arm and round, then a summary line (median Mpixels/s per arm, pitched / packed).  The pitched results are
checked against the packed ones bit for bit.
"""
import argparse
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
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    w, h, B = a.width, a.height, 16
    cam = synth.DEFAULT_CAMERA
    dev = torch.device("cuda", 0)
    depth = torch.stack([torch.from_numpy(synth.make("S2", w, h, seed=0x1234ABCD + f)) for f in range(B)]).to(dev)
    pad = {"packed": 0, "pitched": 16}                          # bytes added to a row
    ao_surf = {k: torch.zeros((B, h, w + p), dtype=torch.uint8, device=dev) for k, p in pad.items()}
    color0 = torch.rand((B, h, w, 4), device=dev).to(torch.float16)
    color = {k: torch.zeros((B, h, w + p // 8, 4), dtype=torch.float16, device=dev) for k, p in pad.items()}
    ao = AmbientOcclusion(w, h, max_batch=B, near_clip=cam.near, far_clip=cam.far, projection00=cam.proj00(w, h))
    stream = torch.cuda.Stream(dev)
    st = stream.cuda_stream
    dptr = [depth[f].data_ptr() for f in range(B)]
    optr = {k: [ao_surf[k][f].data_ptr() for f in range(B)] for k in pad}
    cptr = {k: [color[k][f].data_ptr() for f in range(B)] for k in pad}
    pitches = {k: dict(ao_pitch=(w + p) if p else 0, color_pitch=(w * 8 + p) if p else 0) for k, p in pad.items()}

    def steps(kind, carried, count):
        for _ in range(count):
            ao.execute_device(dptr, optr[kind], st, out_pitch=pitches[kind]["ao_pitch"])      # carries the previous step's composite
            if carried:
                ao.composite_enqueue_device(L.COMPOSITE_MULTIPLY, optr[kind], cptr[kind], **pitches[kind])
            else:
                for f in range(B):
                    ao.composite_device(L.COMPOSITE_MULTIPLY, optr[kind][f], cptr[kind][f], 0, st, **pitches[kind])
        ao.composite_flush(st)

    arms = {f"{kind}_{how}": (kind, how == "carried") for how in ("carried", "separate") for kind in pad}
    res = {k: [] for k in arms}
    lines = []
    same = True
    for r in range(-1, a.rounds):                               # round -1: warm-up
        for name, (kind, carried) in arms.items():
            color[kind][:, :, :w, :] = color0
            torch.cuda.synchronize(dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            steps(kind, carried, a.steps)
            e1.record(stream)
            e1.synchronize()
            if kind == "pitched":
                same = same and torch.equal(color["pitched"][:, :, :w, :], reference) and torch.equal(ao_surf["pitched"][:, :, :w], ao_surf["packed"])
            else:
                reference = color["packed"].clone()
            if r < 0:
                continue
            ms = e0.elapsed_time(e1)
            mpix = w * h * B * a.steps / ms / 1e3
            res[name].append(mpix)
            lines.append({"arm": name, "round": r, "steps": a.steps, "frames_per_step": B, "ms": round(ms, 3), "Mpixels_per_s": round(mpix, 1)})
            print(json.dumps(lines[-1]), flush=True)
    med = {k: statistics.median(v) for k, v in res.items()}
    summary = {"summary": True, "width": w, "height": h, "frames_per_step": B, "row_padding_bytes": pad["pitched"],
               "median_Mpixels_per_s": {k: round(v, 1) for k, v in med.items()},
               "pitched_over_packed_carried": round(med["pitched_carried"] / med["packed_carried"], 4),
               "pitched_over_packed_separate": round(med["pitched_separate"] / med["packed_separate"], 4),
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
