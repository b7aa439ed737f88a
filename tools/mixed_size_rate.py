"""Mixed-size batches (meao_execute_batch_extents): what one call for frames of several sizes costs, S2 frames, R8, HIP events.

    python tools/mixed_size_rate.py [--lib parent/libmeao_hip.so] [--rounds 5] [--ms 150] [--out profiles/mixed_size_rate.jsonl]

Three workloads, each with two arms alternated round by round in one process (an arm runs whole steps until >= --ms of GPU time):
  uniform_4k    16 x 4K.  `extents`: the new entry point with 16 equal extents and params[] (it delegates: the launches of a per-frame call);
                `params`: meao_execute_batch_params of the --lib library (the parent commit's build; this library without --lib).
  main_probes   1 x 4K + 15 x 256 x 256.  `mixed`: one mixed call; `two_calls`: what a host could do before, on a context with
                a reservation of 4K: meao_resize(4K), a call of one frame, meao_resize(256, 256), a call of fifteen (--lib library).
  two_sizes     8 x 4K + 8 x 2560 x 1440, likewise.
Every launch of a mixed call has the grid of its largest frame, and the workgroups beyond a smaller frame's own tiles return at
once: main_probes and two_sizes price those workgroups against the launches they save.  One JSON line per workload, arm and round,
then one summary line per workload (median us per step of each arm and their ratio).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from miniengineao_amd import synth  # noqa: E402
from miniengineao_amd import _lib as L  # noqa: E402

BIG, MID, SMALL = (3840, 2160), (2560, 1440), (256, 256)


def bind(path):
    """The library at `path` with the signatures of every symbol it has (the parent's build lacks the new ones)."""
    if path is None:
        return L.load()
    L.load()                                    # the HIP runtime this process shares with torch, mapped first
    lib = C.CDLL(os.path.abspath(path))
    for name, (restype, argtypes) in L.SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
    return lib


def check(lib, ctx, status):
    if status != L.OK:
        raise RuntimeError("meao status %d: %s" % (status, lib.meao_last_error(ctx).decode()))


def create(lib, w, h, max_batch, reserve=None):
    cam = synth.DEFAULT_CAMERA
    cfg, prm, ctx = L.Config(), L.Params(), C.c_void_p()
    lib.meao_default_config(C.byref(cfg))
    cfg.width, cfg.height, cfg.max_batch = w, h, max_batch
    check(lib, None, lib.meao_create(C.byref(cfg), C.byref(ctx)))
    lib.meao_default_params(C.byref(prm))
    prm.near_clip, prm.far_clip, prm.proj00 = cam.near, cam.far, cam.proj00(w, h)
    check(lib, ctx, lib.meao_set_params(ctx, C.byref(prm)))
    if reserve:
        check(lib, ctx, lib.meao_reserve(ctx, *reserve))
    return ctx, prm


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="the parent commit's libmeao_hip.so for the arms of what a host could do before")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ms", type=float, default=150.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    new, old = bind(None), bind(a.lib)
    stream = torch.cuda.Stream(dev)
    st = C.c_void_p(stream.cuda_stream)

    pool = {}

    def frames(size, n):
        """n device depth frames of `size` (four distinct contents per size, cycled) and n result surfaces."""
        w, h = size
        if size not in pool:
            pool[size] = [torch.from_numpy(synth.make("S2", w, h, seed=0x1234ABCD + k)).to(dev) for k in range(4)]
        depth = [pool[size][f % 4] if f < 4 else pool[size][f % 4].clone() for f in range(n)]
        return depth, [torch.empty((h, w), dtype=torch.uint8, device=dev) for _ in range(n)]

    def ptrs(ts):
        return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])

    def extents(sizes):
        arr = (L.Extent * len(sizes))()
        for f, (w, h) in enumerate(sizes):
            arr[f].width, arr[f].height = w, h
        return arr

    def mixed_arm(sizes, per_frame=False):
        """One meao_execute_batch_extents call for all the frames, on a context of the largest size; per_frame: with the context's
        parameters in every entry of params[] (the call then reads its blocks from the table also where it delegates)."""
        ctx, prm = create(new, *BIG, len(sizes))
        arr = (L.Params * len(sizes))(*[prm] * len(sizes)) if per_frame else None
        by_size = {size: frames(size, sizes.count(size)) for size in dict.fromkeys(sizes)}
        taken = {size: 0 for size in by_size}
        d, o = [], []
        for size in sizes:
            d.append(by_size[size][0][taken[size]])
            o.append(by_size[size][1][taken[size]])
            taken[size] += 1
        pd, po, ext = ptrs(d), ptrs(o), extents(sizes)
        keep = (d, o)

        def step():
            check(new, ctx, new.meao_execute_batch_extents(ctx, len(sizes), pd, po, ext, arr, st))
        return new, ctx, step, keep

    def params_arm(n):
        """meao_execute_batch_params of n 4K frames with the context's parameters in every entry."""
        ctx, prm = create(old, *BIG, n)
        d, o = frames(BIG, n)
        pd, po, arr = ptrs(d), ptrs(o), (L.Params * n)(*[prm] * n)

        def step():
            check(old, ctx, old.meao_execute_batch_params(ctx, n, pd, L.MEM_DEVICE, po, L.MEM_DEVICE, arr, st))
        return old, ctx, step, (d, o)

    def two_calls_arm(groups):
        """One call per size with meao_resize between them, inside a reservation of the largest size."""
        ctx, _ = create(old, *BIG, max(n for _, n in groups), reserve=BIG)
        calls, keep = [], []
        for size, n in groups:
            d, o = frames(size, n)
            keep.append((d, o))
            calls.append((size, n, ptrs(d), ptrs(o)))

        def step():
            for (w, h), n, pd, po in calls:
                check(old, ctx, old.meao_resize(ctx, w, h))
                check(old, ctx, old.meao_execute_batch(ctx, n, pd, L.MEM_DEVICE, po, L.MEM_DEVICE, st))
        return old, ctx, step, keep

    workloads = {
        "uniform_4k": {"extents": lambda: mixed_arm([BIG] * 16, per_frame=True), "params": lambda: params_arm(16)},
        "main_probes": {"mixed": lambda: mixed_arm([BIG] + [SMALL] * 15), "two_calls": lambda: two_calls_arm([(BIG, 1), (SMALL, 15)])},
        "two_sizes": {"mixed": lambda: mixed_arm([BIG] * 8 + [MID] * 8), "two_calls": lambda: two_calls_arm([(BIG, 8), (MID, 8)])},
    }
    lines = []
    for wname, arms in workloads.items():
        built = {name: make() for name, make in arms.items()}
        steps = {}
        for name, (lib, ctx, step, _) in built.items():          # warm-up, and the steps that fill --ms
            for _ in range(3):
                step()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(4):
                step()
            e1.record(stream)
            e1.synchronize()
            steps[name] = max(4, int(a.ms / max(e0.elapsed_time(e1) / 4, 1e-3)) + 1)
        res = {name: [] for name in built}
        for r in range(a.rounds):
            for name, (lib, ctx, step, _) in built.items():
                step()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(steps[name]):
                    step()
                e1.record(stream)
                e1.synchronize()
                ms = e0.elapsed_time(e1)
                res[name].append(ms * 1e3 / steps[name])
                lines.append({"workload": wname, "arm": name, "round": r, "steps": steps[name], "ms": round(ms, 3),
                              "us_per_step": round(res[name][-1], 3)})
                print(json.dumps(lines[-1]), flush=True)
        med = {k: statistics.median(v) for k, v in res.items()}
        first, second = list(med)
        lines.append({"summary": True, "workload": wname, "median_us_per_step": {k: round(v, 2) for k, v in med.items()},
                      "%s_over_%s" % (first, second): round(med[first] / med[second], 4),
                      "other_library": bool(a.lib), "device": torch.cuda.get_device_name(dev)})
        print(json.dumps(lines[-1]), flush=True)
        torch.cuda.synchronize(dev)
        for lib, ctx, _, _ in built.values():
            lib.meao_destroy(ctx)
        pool.clear()
    if a.out:
        with open(a.out, "w") as fh:
            for ln in lines:
                fh.write(json.dumps(ln) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
