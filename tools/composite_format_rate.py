"""The stand-alone composite per colour format: color.rgba *= ao (MULTIPLY) of 16 tightly packed 4K frames with R8 AO, once per
meao_color_format.  HIP events around `steps` passes over the 16 frames.

    python tools/composite_format_rate.py [--rounds 5] [--steps 20] [--arms RGBA16F,RGBA8,...] [--out profiles/composite_format_rate.jsonl]

Five arms (RGBA16F, RGBA32F, RGBA8, R11G11B10F, RGBA8_SRGB), alternated round by round in one process; --arms runs a subset (the
first four against a library older than RGBA8_SRGB, for an A/B).  One JSON line per arm and round, then a summary line: median
Gpixels/s and GB/s per arm -- bytes moved, the colour counted twice (read + write) and the AO once: 17, 33, 9, 9 and 9 bytes per
texel -- and each arm's GB/s over the RGBA16F arm's of the same run, the yardstick (all are the same streaming shape); the
RGBA8_SRGB arm also over the RGBA8 arm's, which moves the same bytes through the same accesses.  The first frame of every arm is
checked against the NumPy model of tests/color_formats.py (RGBA8_SRGB: tests/srgb_format.py) after one pass (the tool runs from a
checkout: it imports the models from the tests package).  Every pass multiplies the same frames in place, so over
the `steps` x rounds passes of an arm the colours decay towards zero (RGBA8 and R11G11B10F reach 0, RGBA32F f32 subnormals): the
later passes move the same bytes with another operand mix.  The colours are reset before every timed round.
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
from tests import color_formats as CF  # noqa: E402
from tests import srgb_format as SF  # noqa: E402

ALL_ARMS = {"RGBA16F": L.COLOR_RGBA16F, "RGBA32F": L.COLOR_RGBA32F, "RGBA8": L.COLOR_RGBA8, "R11G11B10F": L.COLOR_R11G11B10F,
            "RGBA8_SRGB": L.COLOR_RGBA8_SRGB}
ARMS = dict(ALL_ARMS)


def initial(fmt, B, h, w, dev):
    g = torch.Generator(device=dev).manual_seed(1234 + fmt)
    if fmt == L.COLOR_RGBA16F:
        return (torch.rand((B, h, w, 4), device=dev, generator=g) * 4).to(torch.float16)
    if fmt == L.COLOR_RGBA32F:
        return torch.rand((B, h, w, 4), device=dev, generator=g) * 4
    if fmt in (L.COLOR_RGBA8, L.COLOR_RGBA8_SRGB):
        return torch.randint(0, 256, (B, h, w, 4), device=dev, generator=g, dtype=torch.uint8)
    r = torch.randint(0, 0x400, (3, B, h, w), device=dev, generator=g, dtype=torch.int32)        # finite values below 2
    return r[0] | (r[1] << 11) | ((r[2] & 0x1ff) << 22)


def model(fmt, ao, color):
    """One frame through the model; RGBA16F (not one of the model's formats) the same reading with NumPy's own f16 rounding."""
    if fmt == L.COLOR_RGBA16F:
        return (color.astype(np.float32) * CF.ao_to_f32(ao, CF.AO_R8)[..., None]).astype(np.float16).view(np.uint16)
    if fmt == L.COLOR_RGBA8_SRGB:
        return SF.composite(ao, SF.AO_R8, color, fmt, SF.MULTIPLY)[0]
    if fmt == L.COLOR_R11G11B10F:
        color = color.view(np.uint32)
    return CF.composite(ao, CF.AO_R8, color, fmt, CF.MULTIPLY)[0]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--arms", default=",".join(ALL_ARMS))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    for k in list(ARMS):
        if k not in a.arms.split(","):
            del ARMS[k]
    w, h, B = a.width, a.height, 16
    dev = torch.device("cuda", 0)
    aosurf = torch.randint(0, 256, (B, h, w), device=dev, dtype=torch.uint8)
    color0 = {k: initial(f, B, h, w, dev) for k, f in ARMS.items()}
    color = {k: torch.empty_like(v) for k, v in color0.items()}
    ao = AmbientOcclusion(w, h, max_batch=B)
    stream = torch.cuda.Stream(dev)
    st = stream.cuda_stream
    aptr = [aosurf[f].data_ptr() for f in range(B)]
    cptr = {k: [color[k][f].data_ptr() for f in range(B)] for k in ARMS}

    def passes(name, count):
        for _ in range(count):
            for f in range(B):
                ao.composite_device(L.COMPOSITE_MULTIPLY, aptr[f], cptr[name][f], 0, st, color_format=ARMS[name])

    ok = True
    for name, fmt in ARMS.items():                               # one pass, checked
        color[name].copy_(color0[name])
        torch.cuda.synchronize(dev)
        passes(name, 1)
        stream.synchronize()
        got = color[name][0].cpu().numpy()
        want = model(fmt, aosurf[0].cpu().numpy(), color0[name][0].cpu().numpy())
        same = np.array_equal(got.view(np.uint8).reshape(-1), np.ascontiguousarray(want).view(np.uint8).reshape(-1))
        print(json.dumps({"arm": name, "first_frame_equals_the_model": bool(same)}), flush=True)
        ok = ok and same
    res = {k: [] for k in ARMS}
    lines = []
    for r in range(-1, a.rounds):                                # round -1: warm-up
        for name, fmt in ARMS.items():
            color[name].copy_(color0[name])
            torch.cuda.synchronize(dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            passes(name, a.steps)
            e1.record(stream)
            e1.synchronize()
            if r < 0:
                continue
            ms = e0.elapsed_time(e1)
            gpix = w * h * B * a.steps / ms / 1e6
            gbs = gpix * (2 * L.COLOR_TEXEL_BYTES[fmt] + 1)
            res[name].append(gbs)
            lines.append({"arm": name, "round": r, "steps": a.steps, "frames_per_step": B, "ms": round(ms, 3),
                          "Gpixels_per_s": round(gpix, 2), "GB_per_s": round(gbs, 1)})
            print(json.dumps(lines[-1]), flush=True)
    med = {k: statistics.median(v) for k, v in res.items()}
    summary = {"summary": True, "width": w, "height": h, "frames_per_step": B, "ao_format": "R8", "mode": "MULTIPLY",
               "bytes_per_texel": {k: 2 * L.COLOR_TEXEL_BYTES[f] + 1 for k, f in ARMS.items()},
               "median_GB_per_s": {k: round(v, 1) for k, v in med.items()},
               "median_Gpixels_per_s": {k: round(v / (2 * L.COLOR_TEXEL_BYTES[ARMS[k]] + 1), 2) for k, v in med.items()},
               "min_max_GB_per_s": {k: [round(min(v), 1), round(max(v), 1)] for k, v in res.items()},
               "GB_per_s_over_RGBA16F": {k: round(v / med["RGBA16F"], 4) for k, v in med.items()} if "RGBA16F" in med else None,
               "RGBA8_SRGB_GB_per_s_over_RGBA8": round(med["RGBA8_SRGB"] / med["RGBA8"], 4) if "RGBA8_SRGB" in med and "RGBA8" in med else None,
               "results_equal_the_model": ok, "device": torch.cuda.get_device_name(dev)}
    print(json.dumps(summary), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            for ln in lines + [summary]:
                fh.write(json.dumps(ln) + "\n")
    ao.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
