"""FrameStream against the loops it replaces, 4K S2 frames, R8, wall-clock time between two stream synchronisations.

    python tools/frame_stream_rate.py [--rounds 5] [--ms 150] [--host-batch 4] [--out profiles/frame_stream_rate.jsonl]

Two comparisons, the two arms of each alternated round by round in one process (an arm runs whole steps until >= --ms):
  device   16 x 4K device frames per step.  `stream`: FrameStream.run over the tensors, results dropped as they come; `by_hand`:
           the loop of bench.py -- prefetch_device(frames), execute_device(frames, outputs) -- over the same tensors on the same
           torch stream.  The ratio says what the layer costs: result tensors from torch's allocator, one step of look-ahead
           instead of a free-running host, the Python between two calls.
  host     --host-batch x 4K host frames per step (float32: 33 MB each up, 8 MB down).  `stream`: FrameStream.run over NumPy
           arrays; `render_batch`: AmbientOcclusion.render_batch over the same arrays, which stages synchronously.  The ratio
           says what overlapping upload, compute and download gains; both arms are bound by the transfers, not by the kernels.
One JSON line per comparison, arm and round, then one summary line per comparison: median frames per second of each arm and
stream / other.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from miniengineao_amd import AmbientOcclusion, FrameStream, synth  # noqa: E402

W, H = 3840, 2160


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ms", type=float, default=150.0)
    ap.add_argument("--host-batch", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    cam = synth.DEFAULT_CAMERA
    camera = dict(near_clip=cam.near, far_clip=cam.far, projection00=cam.proj00(W, H), reversed_z=cam.reversed_z)
    distinct = [synth.make("S2", W, H, seed=0x1234ABCD + k) for k in range(4)]
    lines = []

    def compare(name, arms, frames_per_step):
        """arms: {arm: run(steps)}; every arm returns with its work complete."""
        steps = {}
        for arm, run in arms.items():
            run(2)                                    # warm-up: allocator, slots, clocks
            t0 = time.perf_counter()
            run(3)
            steps[arm] = max(3, int(a.ms * 1e-3 / max((time.perf_counter() - t0) / 3, 1e-5)) + 1)
        rate = {arm: [] for arm in arms}
        for r in range(a.rounds):
            for arm, run in arms.items():
                run(1)
                t0 = time.perf_counter()
                run(steps[arm])
                s = time.perf_counter() - t0
                rate[arm].append(frames_per_step * steps[arm] / s)
                lines.append({"comparison": name, "arm": arm, "round": r, "steps": steps[arm], "ms": round(s * 1e3, 3),
                              "frames_per_s": round(rate[arm][-1], 2)})
                print(json.dumps(lines[-1]), flush=True)
        med = {arm: statistics.median(v) for arm, v in rate.items()}
        first, second = list(med)
        lines.append({"summary": True, "comparison": name, "frames_per_step": frames_per_step,
                      "median_frames_per_s": {k: round(v, 2) for k, v in med.items()},
                      "median_Mpixels_per_s": {k: round(v * W * H / 1e6, 1) for k, v in med.items()},
                      "%s_over_%s" % (first, second): round(med[first] / med[second], 4), "device": torch.cuda.get_device_name(dev)})
        print(json.dumps(lines[-1]), flush=True)

    with torch.cuda.stream(torch.cuda.Stream(dev)):   # both arms of a comparison on this one torch stream
        stream = torch.cuda.current_stream(dev)
        # ---- device frames
        B = 16
        depth = [torch.from_numpy(distinct[f % 4]).to(dev) for f in range(B)]
        outs = [torch.empty((H, W), dtype=torch.uint8, device=dev) for _ in range(B)]
        dptr, optr = [t.data_ptr() for t in depth], [t.data_ptr() for t in outs]
        fs = FrameStream(W, H, batch=B, **camera)
        ao = AmbientOcclusion(W, H, max_batch=B, pipelined=True, **camera)

        def device_stream(steps):
            for _ in fs.run(depth[f % B] for f in range(steps * B)):
                pass
            stream.synchronize()

        def device_by_hand(steps):
            for _ in range(steps):
                ao.prefetch_device(dptr)
                ao.execute_device(dptr, optr, stream.cuda_stream)
            stream.synchronize()

        compare("device", {"stream": device_stream, "by_hand": device_by_hand}, B)
        same = all(torch.equal(r, o) for r, o in zip(fs.run(depth), outs))
        print(json.dumps({"comparison": "device", "results_equal": same}), flush=True)
        fs.close()
        ao.close()
        del depth, outs
        # ---- host frames
        B = a.host_batch
        fs = FrameStream(W, H, batch=B, **camera)
        ao = AmbientOcclusion(W, H, max_batch=B, **camera)
        host = [distinct[f % 4] for f in range(B)]

        def host_stream(steps):
            for _ in fs.run(host[f % B] for f in range(steps * B)):
                pass

        def host_render_batch(steps):
            for _ in range(steps):
                ao.render_batch(host)

        compare("host", {"stream": host_stream, "render_batch": host_render_batch}, B)
        fs.close()
        ao.close()
    if a.out:
        with open(a.out, "w") as fh:
            for ln in lines:
                fh.write(json.dumps(ln) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
