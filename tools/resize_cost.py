"""Dynamic resolution: what a size change costs the host and a pipelined stream, 16 frames per step, S2 frames, sizes 3840 x 2160 and
2560 x 1440.

    python tools/resize_cost.py [--lib PATH] [--rounds 5] [--steps 40] [--resizes 40] [--reserved-first] [--out profiles/resize_cost.jsonl]

--lib: another build of libmeao_hip.so (e.g. the parent commit's, built at the same path): a library without meao_reserve runs the
arms that need no reservation only.  Arms, alternated round by round in one process:
  resize_host     host time of one meao_resize (time.perf_counter_ns around the call) between the two sizes, both directions, on a
                  context with a 16-frame execute in flight on its stream; `reserved` (meao_reserve(3840, 2160) first) and `exact_fit`
  alternating     a pipelined stream whose size alternates every step.  `reserved`: meao_prefetch_batch_sized(next) ->
                  meao_execute_batch(current) -> meao_resize(next).  `exact_fit`: meao_resize(next) drops every announcement, and none
                  can be made for another size, so the loop is meao_execute_batch -> meao_resize.  Wall clock around the steps with
                  one stream synchronisation at the end (a resize that blocks the host is part of what is measured); ms per pair of
                  steps (one of each size)
  constant        meao_prefetch_batch -> meao_execute_batch at 3840 x 2160, HIP events; `reserved` and `exact_fit`: the same device
                  code either way, the difference is host time
--reserved-first creates (and runs, in every round) the reserved context before the exact-fit one: the two arenas are separate
allocations of the same size, and which of them a context gets is the only thing that differs between the `constant` arms.
One JSON line per arm and round, then a summary line (medians).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from miniengineao_amd import synth  # noqa: E402
from miniengineao_amd import _lib as L  # noqa: E402
from miniengineao_amd import codehash  # noqa: E402

BIG, SMALL, B = (3840, 2160), (2560, 1440), 16


def load(path):
    """The library's C ABI without insisting on the symbols this tree added (another commit's build has fewer)."""
    L._share_torch_hip_runtime()
    lib = C.CDLL(path)
    for name, (restype, argtypes) in L.SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = restype, argtypes
    return lib


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=L.LIB_PATH)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--resizes", type=int, default=40)
    ap.add_argument("--reserved-first", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = load(a.lib)
    can_reserve = hasattr(lib, "meao_reserve")
    cam = synth.DEFAULT_CAMERA
    dev = torch.device("cuda", 0)

    def check(rc, ctx):
        if rc != L.OK:
            raise RuntimeError(lib.meao_last_error(ctx).decode())

    # four distinct frames per size, dealt round the 16 slots of two batches
    P = C.c_void_p * B
    pin, pout, keep = {}, {}, []
    for size in (BIG, SMALL):
        w, h = size
        distinct = [torch.from_numpy(synth.make("S2", w, h, seed=0x1234ABCD + f)).to(dev) for f in range(4)]
        sets = [torch.stack([distinct[(f + k) % 4] for f in range(B)]) for k in range(2)]
        out = torch.zeros((B, h, w), dtype=torch.uint8, device=dev)
        keep += [sets, out]
        pin[size] = [P(*[s[f].data_ptr() for f in range(B)]) for s in sets]
        pout[size] = P(*[out[f].data_ptr() for f in range(B)])
    stream = torch.cuda.Stream(dev)
    st = C.c_void_p(stream.cuda_stream)

    def context(reserved):
        cfg = L.Config()
        lib.meao_default_config(C.byref(cfg))
        cfg.width, cfg.height, cfg.max_batch, cfg.pipelined = BIG[0], BIG[1], B, 1
        ctx = C.c_void_p()
        check(lib.meao_create(C.byref(cfg), C.byref(ctx)), None)
        prm = L.Params()
        lib.meao_default_params(C.byref(prm))
        prm.near_clip, prm.far_clip, prm.proj00 = cam.near, cam.far, cam.proj00(*BIG)
        check(lib.meao_set_params(ctx, C.byref(prm)), ctx)
        if reserved:
            check(lib.meao_reserve(ctx, BIG[0], BIG[1]), ctx)
        return ctx

    def execute(ctx, size, k):
        check(lib.meao_execute_batch(ctx, B, pin[size][k & 1], L.MEM_DEVICE, pout[size], L.MEM_DEVICE, st), ctx)

    def resize_host(ctx):
        """[(direction, ns)] of a.resizes resizes, each with the execute before it still in flight"""
        out = []
        size = BIG
        for k in range(a.resizes):
            execute(ctx, size, k)
            nxt = SMALL if size == BIG else BIG
            t0 = time.perf_counter_ns()
            rc = lib.meao_resize(ctx, nxt[0], nxt[1])
            t1 = time.perf_counter_ns()
            check(rc, ctx)
            out.append(("down" if nxt == SMALL else "up", t1 - t0))
            size = nxt
        if size != BIG:
            check(lib.meao_resize(ctx, BIG[0], BIG[1]), ctx)
        stream.synchronize()
        return out

    def alternating(ctx, reserved):
        """ms per pair of steps"""
        stream.synchronize()
        size = BIG
        t0 = time.perf_counter()
        for k in range(a.steps):
            nxt = SMALL if size == BIG else BIG
            if reserved:
                check(lib.meao_prefetch_batch_sized(ctx, nxt[0], nxt[1], B, pin[nxt][(k + 1) & 1], 0, None), ctx)
            execute(ctx, size, k)
            check(lib.meao_resize(ctx, nxt[0], nxt[1]), ctx)
            size = nxt
        stream.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        if size != BIG:
            check(lib.meao_resize(ctx, BIG[0], BIG[1]), ctx)
        return ms / (a.steps / 2)

    def constant(ctx):
        """us per frame"""
        check(lib.meao_prefetch_batch(ctx, B, pin[BIG][1]), ctx)
        execute(ctx, BIG, 0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for k in range(1, a.steps + 1):
            check(lib.meao_prefetch_batch(ctx, B, pin[BIG][(k + 1) & 1]), ctx)
            execute(ctx, BIG, k)
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / (a.steps * B)

    kinds = ["exact_fit"] + (["reserved"] if can_reserve else [])
    if a.reserved_first:
        kinds.reverse()
    ctxs = {kind: context(kind == "reserved") for kind in kinds}
    for ctx in ctxs.values():           # warm-up
        constant(ctx)
    res, lines = {}, []

    def note(arm, kind, value, unit, r):
        res.setdefault((arm, kind), []).append(value)
        lines.append({"arm": arm, "context": kind, "round": r, unit: round(value, 3)})
        print(json.dumps(lines[-1]), flush=True)

    for r in range(a.rounds):
        for kind, ctx in ctxs.items():
            per = resize_host(ctx)
            for d in ("down", "up"):
                note("resize_host_" + d, kind, statistics.median(ns for dd, ns in per if dd == d) / 1e3, "median_us", r)
            note("alternating", kind, alternating(ctx, kind == "reserved"), "ms_per_pair_of_steps", r)
            note("constant", kind, constant(ctx), "us_per_frame", r)
    summary = {"summary": True, "library": os.path.basename(a.lib), "device_code_sha256": codehash.device_code_sha256(a.lib),
               "has_meao_reserve": can_reserve, "context_order": kinds, "frames_per_step": B, "sizes": [BIG, SMALL], "steps": a.steps, "resizes": a.resizes,
               "median": {"%s/%s" % k: round(statistics.median(v), 3) for k, v in sorted(res.items())},
               "device": torch.cuda.get_device_name(dev)}
    print(json.dumps(summary), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            for ln in lines + [summary]:
                fh.write(json.dumps(ln) + "\n")
    for ctx in ctxs.values():
        lib.meao_destroy(ctx)
    return 0


if __name__ == "__main__":
    sys.exit(main())
