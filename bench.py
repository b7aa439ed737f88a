#!/usr/bin/env python3
"""bench.py -- throughput of the multi-scale SSAO hot path on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload 4k|1080p|8k] [--batch B]
    python bench.py --pool G          # one process driving G pool members through meao_pool_* (in-process host)

A step = one pass of the full pipeline (downsample -> render x4 levels -> upsample x4) over
one batch of B independent synthetic frames, depth already resident in HBM.  Prints ONE JSON
line: Mpixels/s (whole job, all ranks), the roofline of the dominant kernel measured live
with HIP events on the launch stream, and the CPU oracle timed on the host cores (rank 0,
N=1 only) as a reported baseline.  The outputs of the TIMED (pipelined) path are validated
against the CPU oracle right after the timed region, before anything else runs.

N>1: launched by torch.distributed.run, one rank per GPU; frames are sharded across ranks
(weak scaling: B frames per rank), there is no data-path collective -- RCCL is used only for
the barrier and the max-over-ranks of the timed region.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import torch  # before libmeao_hip.so: both then share torch's libamdhip64 (see _lib.py)

from miniengineao_amd import AmbientOcclusion, AmbientOcclusionPool, _lib, synth
from miniengineao_amd import distributed as mdist
from miniengineao_amd import topology
from miniengineao_amd.sharding import frame_checksum, frame_seed, frames_for_rank

HBM_PEAK_GBPS = 8000.0      # MI355X HBM3E spec peak (MI355X_MICROARCH.md chip table)
HBM_COPY_CEILING_GBPS = 6290.0
# VALU issue roof (MI355X_MICROARCH.md chip table): 256 CUs x 4 SIMDs, one wave64 v_fma_f32 per 2 cycles and SIMD, 2.4 GHz spec clock
# (the clock a kernel really ran at is a few percent lower: GRBM_GUI_ACTIVE / 8 / duration of the PMC passes says ~2.3 GHz under
# the render kernel; the SPEC clock is used here, so valu_frac is a lower bound of the issue-slot use)
VALU_PEAK_WAVE_INSTS_PER_S = 256 * 4 * 2.4e9 / 2.0
# What the instruction mix of the north-star sub-path allows at best (tools/ubench_issue.hip): ~380 M VALU
# wave-instructions per 16 4K frames, every one needed for a bit-exact result, issuing at 2.4 - 2.7 cycles each if nothing ever waited
SUBPATH_VALU_FLOOR_FRAC_OF_HBM_ROOFLINE = 0.38

WORKLOADS = {
    # name: (W, H, generator, camera, intensity, ao_format, description)
    "4k": (3840, 2160, "S2", synth.DEFAULT_CAMERA, 1.0, _lib.AO_R8,
           "4K (3840x2160) S2 synthetic depth, full 4-level pipeline, R8 AO"),
    "1080p": (1920, 1080, "S3", synth.SPONZA_CAMERA, 1.1, _lib.AO_R8,
              "1080p S3 Sponza-like atrium (substitute for captured Sponza depth), full 4-level pipeline, R8 AO"),
    "8k": (7680, 4320, "S2", synth.DEFAULT_CAMERA, 1.0, _lib.AO_F16,
           "8K (7680x4320) S2 synthetic depth, full 4-level pipeline, fp16 AO storage"),
}


def make_frame(kind: str, w: int, h: int, seed: int, index: int = 0) -> np.ndarray:
    """Global frame `index` of a workload.  S3: frame 0 is the plain atrium (the stand-in for the captured Sponza
    depth), every other frame the same scene with seeded boxes in front of it -- distinct frames, so that a
    frame-index mix-up shows in the per-frame checksums."""
    if kind == "S3":
        return synth.atrium(w, h) if index == 0 else synth.atrium_with_occluders(w, h, seed)
    return synth.make(kind, w, h, seed=seed)


def default_batch(w: int, h: int) -> int:
    """133 Mpixels per step on every workload: 64 frames at 1080p, 16 at 4K, 4 at 8K."""
    return max(1, min((3840 * 2160 * 16) // (w * h), _lib.MAX_BATCH))


def oracle_settings(w, h, cam, intensity, ao_format, hq_levels=0, exhaustive=False):
    from oracle import oracle as O   # test infrastructure: the checker / reported baseline, never the thing measured
    return O, O.Settings(w, h, proj00=cam.proj00(w, h), near_clip=cam.near, far_clip=cam.far,
                         reversed_z=cam.reversed_z, intensity=intensity, ao_format=ao_format, hq_levels=hq_levels,
                         sample_set=O.SAMPLES_EXHAUSTIVE if exhaustive else O.SAMPLES_CHECKER)


def cpu_baseline(w, h, cam, intensity, ao_format, depth, budget_s=20.0):
    """The oracle (a port of the reference passes), row-parallel on all host cores, timed on a
    bounded sample of the same workload: whole frames of this workload, median of <=8 after
    one warm-up, stopping early once ~budget_s of CPU time is spent."""
    O, s = oracle_settings(w, h, cam, intensity, ao_format)
    cores = O.host_cores()           # affinity mask capped by the cgroup CPU quota: what this process can really use
    times = []
    t_begin = time.perf_counter()
    O.run(depth, s, nthreads=cores, result_only=True)       # warm-up
    for _ in range(8):
        t0 = time.perf_counter()
        O.run(depth, s, nthreads=cores, result_only=True)
        times.append(time.perf_counter() - t0)
        if time.perf_counter() - t_begin > budget_s:
            break
    med = float(np.median(times))
    t0 = time.perf_counter()
    O.run(depth, s, nthreads=1, result_only=True)           # the same frame on one core (scalar C)
    single = time.perf_counter() - t0
    return {"value": round(w * h / med / 1e6, 3), "unit": "Mpixels/s", "cores": cores, "kind": "port",
            "single_core_value": round(w * h / single / 1e6, 3),
            "host_logical_cpus": os.cpu_count(),
            "sample": f"{len(times)} timed full {w}x{h} frame(s) of the bench workload after 1 warm-up, "
                      f"median; C oracle (oracle/meao_oracle.c) row-parallel on {cores} threads = the CPUs this process may use "
                      f"(affinity mask capped by the cgroup quota; the host shows {os.cpu_count()} logical CPUs)",
            "seconds_per_frame": round(med, 4),
            "thread_scaling": round(single / med, 1),
            "note": "a reported baseline, never a target: the port is row-parallel per pass (persistent thread pool drawing chunks "
                    f"of rows, a join between the ~25 passes of a frame) and scales {single / med:.1f}x on {cores} threads; "
                    "kernel quality is judged by the roofline fraction, not by the GPU / CPU ratio"}


_CODE_SHA = []


def loaded_code_sha256() -> str:
    if not _CODE_SHA:
        from miniengineao_amd import codehash
        _CODE_SHA.append(codehash.device_code_sha256(_lib.LIB_PATH))
    return _CODE_SHA[0]


def traffic_bytes(traffic):
    """Bytes of a pmc_traffic() record, None when there is none or it belongs to another build."""
    return traffic["bytes"] if traffic and not traffic.get("stale") and traffic.get("bytes") else None


def pmc_traffic(workload: str, kernel: str, frames_per_launch: int):
    """HBM-side bytes per launch of `kernel` from the COMMITTED rocprofv3 --pmc passes
    (profiles/pmc_traffic.json: FETCH_SIZE / WRITE_SIZE collected in separate runs by
    tools/run_pmc.sh, corrected as MI355X_MICROARCH.md prescribes; per frame, scaled here by the
    frames per launch).  Not measured in the run that prints it -- the `source` says so.
    None when no measurement exists for this workload/kernel."""
    path = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    try:
        table = json.load(open(path))
        row = table[workload][kernel]
        # the counters belong to ONE build of the kernels: the device code (.hip_fatbin) they were collected from is hashed into the
        # file; a library whose device code differs gets no traffic figure from it
        measured_on = table.get("_code_sha256", {}).get(workload)
        if measured_on != loaded_code_sha256():
            return {"stale": True, "bytes": None,
                    "source": f"profiles/pmc_traffic.json holds counters of device code {str(measured_on)[:12]}..., the loaded library is "
                              f"{loaded_code_sha256()[:12]}...: not applicable to this build (re-run tools/run_pmc.sh + tools/make_pmc_traffic.py)"}
        out = {"stale": False, "bytes": int(row["bytes_per_frame"] * frames_per_launch),
               "source": f"committed PMC pass {table.get('_tags', {}).get(workload, table.get('_tag', '(untagged)'))} in profiles/pmc_traffic.json -- "
                         "separate rocprofv3 --pmc runs, NOT measured in this run",
               "note": row.get("note", "")}
        if "valu_wave_insts_per_frame" in row:      # SQ_INSTS_VALU of the same PMC passes
            out["valu_wave_insts"] = int(row["valu_wave_insts_per_frame"] * frames_per_launch)
        return out
    except (OSError, KeyError, ValueError):
        return None


# Per-pass HIP events in EVERY step of a timed region.  (meao_set_profiling(N) can sample every Nth step, and the event records cost
# 1 - 4 % of a step -- `without_pass_events` -- but a sampled step is not a typical one: the markers of the one evented step in four
# stall a front end that otherwise runs ahead, render reads 183 us instead of 169 and the kernels' sum exceeds the step.  Every
# step evented is self-consistent: sum of kernels <= step.)
PASS_EVENT_PERIOD = 1


PMC_ROW_OF = {"upsample_L2_to_L1": "upsample_blend_passes", "upsample_L3_to_L2": "upsample_blend_passes", "upsample_L4_to_L3": "upsample_blend_passes"}


def pass_table(ao, pass_ms, B, pipelined, workload=None, ceiling_gbps=None):
    """Per-launch roofline rows: algorithmic bytes of what each launch carries / its HIP-event duration; with `workload`, next
    to them the VALU issue fraction (committed SQ_INSTS_VALU of the launch / its duration / the VALU issue roof), the fraction of
    the copy ceiling its moved bytes reach, and which of the two is larger (`limiter`)."""
    alg = ao.algorithmic_bytes()                 # per frame, reference storage formats
    names = list(_lib.PASS_NAMES)
    if pipelined:
        # the downsample pass of the next step runs inside the last upsample kernel: its bytes move there
        u0, d0 = names.index("upsample_L1_to_L0"), names.index("downsample")
        if pass_ms[d0] <= 0:
            alg[u0] += alg[d0]
            alg[d0] = 0
            names[u0] = "upsample_L1_to_L0+downsample_next"
    u3, u2 = names.index("upsample_L4_to_L3"), names.index("upsample_L3_to_L2")
    if pass_ms[u3] <= 0 < pass_ms[u2]:
        # the library evaluates L4 -> L3 inside the L3 -> L2 launch (upsample_two_level_kernel): its bytes move there
        alg[u2] += alg[u3]
        alg[u3] = 0
        names[u2] = "upsample_L4_to_L3+L3_to_L2"
    u1 = names.index("upsample_L2_to_L1")
    if pass_ms[u3] <= 0 and pass_ms[u2] <= 0 < pass_ms[u1] and alg[u2] > 0:
        # small calls: all three blend passes run inside the L2 -> L1 launch (upsample_three_level_kernel)
        alg[u1] += alg[u2] + alg[u3]
        alg[u2] = alg[u3] = 0
        names[u1] = "upsample_L4_to_L3+L3_to_L2+L2_to_L1"
    rows = []
    for k in range(_lib.NUM_PASSES):
        if pass_ms[k] <= 0:
            continue
        gbps = alg[k] * B / (pass_ms[k] * 1e-3) / 1e9
        row = {"kernel": names[k], "ms": round(pass_ms[k], 5), "algorithmic_MB": round(alg[k] * B / 1e6, 3),
               "GBps": round(gbps, 1), "frac": round(gbps / HBM_PEAK_GBPS, 4)}
        if workload is not None:
            row.update(limiter_fields(pmc_traffic(workload, PMC_ROW_OF.get(names[k], names[k]), B), pass_ms[k], ceiling_gbps))
        rows.append(row)
    return rows, alg, names


def limiter_fields(traffic, launch_ms, ceiling_gbps):
    """valu_frac / moved_bytes_vs_copy_ceiling / limiter of one launch from its committed PMC record (None when there is none for
    this build): limiter = whichever of the two fractions is larger."""
    out = {"valu_frac": None, "moved_bytes_vs_copy_ceiling": None, "limiter": None}
    if not traffic or traffic.get("stale"):
        return out
    if traffic.get("valu_wave_insts"):
        out["valu_frac"] = round(traffic["valu_wave_insts"] / (launch_ms * 1e-3) / VALU_PEAK_WAVE_INSTS_PER_S, 4)
    if traffic.get("bytes") and ceiling_gbps:
        out["moved_bytes_vs_copy_ceiling"] = round(traffic["bytes"] / (launch_ms * 1e-3) / 1e9 / ceiling_gbps, 4)
    if out["valu_frac"] is not None and out["moved_bytes_vs_copy_ceiling"] is not None:
        out["limiter"] = "valu" if out["valu_frac"] >= out["moved_bytes_vs_copy_ceiling"] else "hbm"
    return out


class Workload:
    """One workload resident on this rank's GPU: frames, outputs, context(s), the step function."""

    def __init__(self, name, args, dev, local_rank, rank, world, batch=None, in_flight=1):
        self.name = name
        self.w, self.h, self.kind, self.cam, self.intensity, self.ao_format, self.desc = WORKLOADS[name]
        if args.ao_format is not None and name == args.workload:
            self.ao_format = _lib.AO_R8 if args.ao_format == "r8" else _lib.AO_F16
            self.desc = self.desc.replace("fp16 AO storage", "AO").replace("R8 AO", "AO") + \
                (", R8 storage" if self.ao_format == _lib.AO_R8 else ", fp16 storage")
        self.hq_levels = args.hq_levels if name == args.workload else 0
        self.exhaustive = args.exhaustive if name == args.workload else False
        if self.hq_levels:
            self.desc += f", VARIANT hq_levels={self.hq_levels}"
        if self.exhaustive:
            self.desc += ", VARIANT 68-sample set"
        w, h = self.w, self.h
        self.B = max(1, min(batch if batch is not None else default_batch(w, h), _lib.MAX_BATCH))
        self.dev, self.world = dev, world
        ao_dtype = torch.uint8 if self.ao_format == _lib.AO_R8 else torch.int16
        # synthetic frames of this rank, resident in HBM: global frame g goes to rank g mod world
        # (miniengineao_amd.sharding.frames_for_rank), weak scaling: B frames per rank
        self.my_frames = frames_for_rank(world * self.B, rank, world)
        self.frames = [make_frame(self.kind, w, h, frame_seed(0x1234ABCD, g), g) for g in self.my_frames]
        self.depth_dev = [torch.from_numpy(f).to(dev) for f in self.frames]
        self.nfl = max(1, in_flight)
        self.out_dev = [[torch.empty((h, w), dtype=ao_dtype, device=dev) for _ in range(self.B)] for _ in range(self.nfl)]
        self.pipelined = not args.no_pipeline
        self.ctxs = []
        for _ in range(self.nfl):
            c = AmbientOcclusion(w, h, device=local_rank, num_levels=4, ao_format=self.ao_format, max_batch=self.B,
                                 near_clip=self.cam.near, far_clip=self.cam.far, projection00=self.cam.proj00(w, h),
                                 reversed_z=self.cam.reversed_z, hq_levels=self.hq_levels,
                                 sample_set=_lib.SAMPLES_EXHAUSTIVE if self.exhaustive else _lib.SAMPLES_CHECKER,
                                 pipelined=self.pipelined)
            c.intensity = self.intensity
            if args.roctx:
                c.set_tracing(True)
            if args.blend_tall_min_tiles is not None:
                c.debug_set(_lib.DEBUG_BLEND_TALL_MIN_TILES, args.blend_tall_min_tiles)
            self.ctxs.append(c)
        self.ao = self.ctxs[0]
        tstreams = [torch.cuda.current_stream(dev)] + [torch.cuda.Stream(dev) for _ in range(self.nfl - 1)]
        self.streams = [t.cuda_stream for t in tstreams]
        self.dptr = [t.data_ptr() for t in self.depth_dev]
        self.optrs = [[t.data_ptr() for t in outs] for outs in self.out_dev]
        self.counter = 0
        self.use_prefetch = self.pipelined

    def step(self):
        k = self.counter % self.nfl
        self.counter += 1
        if self.use_prefetch:
            # streaming use: the frames of this context's NEXT step are announced, so this step's last
            # kernel also runs their downsample pass (every step still does one downsample pass of work)
            self.ctxs[k].prefetch_device(self.dptr)
        self.ctxs[k].execute_device(self.dptr, self.optrs[k], self.streams[k])

    def fence(self):
        mdist.fence(self.dev)     # synchronize + barrier + synchronize

    def last_outputs(self):
        return self.out_dev[(self.counter - 1) % self.nfl]

    def ramp(self, seconds):
        # clock ramp: untimed back-to-back work before the warm-up steps.  The chip's clocks and power state
        # settle slowly: in the rocprofv3 trace of this command the render kernel goes 260 -> 200 -> 185 ->
        # 178 us over the first 40 ms of continuous load (profiles/README.md), so a run with a small
        # --steps / --warmup would otherwise be timed on the slope.
        t_ramp = time.perf_counter()
        while time.perf_counter() - t_ramp < seconds:
            for _ in range(8):
                self.step()
            torch.cuda.synchronize(self.dev)

    def timed(self, steps, warmup, pass_events=True, pass_mask=0):
        """W warm-up steps, then exactly `steps` steps between two fences, per-pass HIP events on (pass_events=False: off --
        the library then puts nothing but its kernels on the stream; pass_mask: only those launch slots are bracketed).
        Returns (elapsed max over ranks, own elapsed, pass_ms, event samples)."""
        for _ in range(warmup):
            self.step()
        # HIP events around every pass of every step (PASS_EVENT_PERIOD = 1), on the launch stream
        for c in self.ctxs:
            c.debug_set(_lib.DEBUG_PROFILE_PASS_MASK, pass_mask)
            c.set_profiling(PASS_EVENT_PERIOD if pass_events else 0)
        self.fence()
        t0 = time.perf_counter()
        for _ in range(steps):
            self.step()
        self.fence()
        mine = time.perf_counter() - t0
        per_ctx = [c.pass_times_ms() for c in self.ctxs]
        samples = sum(n for _, n in per_ctx)
        pass_ms = [sum(ms[k] * n for ms, n in per_ctx) / max(samples, 1) for k in range(_lib.NUM_PASSES)]
        for c in self.ctxs:
            c.set_profiling(False)
        return mdist.max_over_ranks(mine, self.dev), mine, pass_ms, samples

    def steps_for(self, min_time_ms, steps):
        """Raise `steps` so that the timed region lasts at least min_time_ms; all ranks agree (max of the estimates)."""
        if min_time_ms <= 0:
            return steps
        self.fence()
        t_est = time.perf_counter()
        for _ in range(3):
            self.step()
        self.fence()
        est = mdist.max_over_ranks((time.perf_counter() - t_est) / 3.0, self.dev)
        return max(steps, int(np.ceil(min_time_ms * 1e-3 / max(est, 1e-6))))

    def validate(self, frames_vs_oracle):
        """Outside every timed region: one checksum per output frame of the LAST step, gathered over RCCL, and
        `frames_vs_oracle` frames of this rank compared bit for bit with the CPU oracle."""
        torch.cuda.synchronize(self.dev)
        outs = self.last_outputs()
        host = [t.cpu().numpy() for t in outs]
        sums = [frame_checksum(a) for a in host]
        all_sums = mdist.gather_checksums(sums, self.dev)
        validated = mismatched = 0
        if frames_vs_oracle > 0:
            O, s = oracle_settings(self.w, self.h, self.cam, self.intensity, self.ao_format, self.hq_levels, self.exhaustive)
            order = list(dict.fromkeys([0, self.B - 1] + list(range(self.B))))      # first, last, then the rest
            threads = max(1, O.host_cores() // max(self.world, 1))
            for f in sorted(order[:frames_vs_oracle]):
                want = O.run(self.frames[f], s, nthreads=threads, result_only=True)["result"]
                validated += 1
                mismatched += int(not np.array_equal(host[f].view(want.dtype), want))
        v = mdist.gather_floats(float(validated), self.dev), mdist.gather_floats(float(mismatched), self.dev)
        return {"frames_checksummed": sum(len(r) for r in all_sums),
                "distinct_checksums": len({c for r in all_sums for c in r}),
                "frames_vs_oracle": int(sum(v[0])), "mismatching_frames": int(sum(v[1]))}, all_sums

    def close(self):
        for c in self.ctxs:
            c.close()
        self.ctxs = []


def measure_other_workload(name, args, dev, local_rank, ceiling_gbps=None):
    """A short sub-measurement of another BASELINE single-GPU configuration inside the default line, so that the
    driver's record covers all three (1080p Sponza-like S3, 8K fp16): pipelined timed region of >= 10 steps,
    validated against the oracle, and a plain-sequence leg for the render + upsample sub-path."""
    wl = Workload(name, args, dev, local_rank, 0, 1)
    try:
        wl.ramp(0.040)
        steps = wl.steps_for(30.0, 10)
        elapsed, _, pass_ms, _ = wl.timed(steps, 3)
        check, _ = wl.validate(1 if name == "8k" else 2)
        rows, alg, names = pass_table(wl.ao, pass_ms, wl.B, wl.pipelined, name, ceiling_gbps)
        dom = max(rows, key=lambda r: r["ms"])
        traffic = pmc_traffic(name, dom["kernel"], wl.B)       # committed PMC pass of THIS workload (profiles/pmc_traffic.json)
        dom_real = None if traffic_bytes(traffic) is None else round(traffic_bytes(traffic) / (dom["ms"] * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4)
        out = {"workload": wl.desc, "frames_per_step": wl.B, "steps": steps,
               "value": round(float(wl.w) * wl.h * wl.B * steps / elapsed / 1e6, 1), "unit": "Mpixels/s",
               "ms_per_step": round(elapsed / steps * 1e3, 4),
               "dominant": {"kernel": dom["kernel"], "frac": dom["frac"], "ms": dom["ms"], "real_traffic_frac": dom_real,
                            "traffic": traffic},
               "whole_frame_frac": round(sum(wl.ao.algorithmic_bytes()) * wl.B / (elapsed / steps) / 1e9 / HBM_PEAK_GBPS, 4),
               "passes": rows, "validation_pipelined": check}
        if wl.pipelined:
            wl.use_prefetch = False
            wl.ramp(0.020)
            pel, _, plain_ms, _ = wl.timed(steps, 3)
            ren_ups_bytes = sum(wl.ao.algorithmic_bytes()[1:])
            ren_ups_ms = sum(plain_ms[1:])
            out["plain_launch_sequence"] = {"value": round(float(wl.w) * wl.h * wl.B * steps / pel / 1e6, 1),
                                            "ms_per_step": round(pel / steps * 1e3, 4)}
            out["render_plus_upsample_frac"] = round(ren_ups_bytes * wl.B / (ren_ups_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4)
            out["validation_plain"] = wl.validate(1)[0]
        return out
    finally:
        wl.close()


def measure_pool(args, G, B=None, ramp_s=0.080) -> dict:
    """The in-process host of DESIGN.md section 7: ONE process drives G pool members through the C ABI
    (meao_pool_prefetch_batch + meao_pool_execute_batch), member m on device m mod (visible devices) --
    all on device 0 on a 1-GPU box, devices 0..G-1 on a real node.  Same step, same JSON as the
    one-process-per-GPU launch; `per_member_ms` = each member's own kernel time per step (HIP events)."""
    import ctypes as C
    ndev = torch.cuda.device_count()
    devices = [m % ndev for m in range(G)]
    w, h, kind, cam, intensity, ao_format, desc = WORKLOADS[args.workload]
    if B is None:
        B = args.batch if args.batch is not None else default_batch(w, h)
    B = max(1, min(B, _lib.MAX_BATCH))
    n = B * G
    ao_dtype = torch.uint8 if ao_format == _lib.AO_R8 else torch.int16
    frames = [make_frame(kind, w, h, frame_seed(0x1234ABCD, g), g) for g in range(n)]
    depth_dev = [torch.from_numpy(frames[g]).to(torch.device("cuda", devices[g % G])) for g in range(n)]   # frame g lives where member g mod G runs
    out_dev = [torch.empty((h, w), dtype=ao_dtype, device=torch.device("cuda", devices[g % G])) for g in range(n)]
    pipelined = not args.no_pipeline
    pool = AmbientOcclusionPool(w, h, devices, max_batch=B, ao_format=ao_format, near_clip=cam.near, far_clip=cam.far,
                                projection00=cam.proj00(w, h), reversed_z=cam.reversed_z, intensity=intensity,
                                pipelined=pipelined)
    lib = _lib.load()
    dptr, optr = [t.data_ptr() for t in depth_dev], [t.data_ptr() for t in out_dev]

    def sync_all():
        for d in sorted(set(devices)):
            torch.cuda.synchronize(torch.device("cuda", d))
        pool.synchronize()

    def step():
        if pipelined:
            pool.prefetch_device(dptr)
        pool.execute_device(dptr, optr)

    sync_all()
    t_ramp = time.perf_counter()
    while time.perf_counter() - t_ramp < ramp_s:
        for _ in range(4):
            step()
        pool.synchronize()
    for _ in range(args.warmup):
        step()
    sync_all()
    steps = args.steps
    if args.min_time_ms > 0:
        t_est = time.perf_counter()
        for _ in range(3):
            step()
        sync_all()
        steps = max(steps, int(np.ceil(args.min_time_ms * 1e-3 / max((time.perf_counter() - t_est) / 3.0, 1e-6))))
    for m in range(G):
        _lib.check(lib.meao_set_profiling(pool.member_context(m), PASS_EVENT_PERIOD))
    sync_all()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    sync_all()
    elapsed = time.perf_counter() - t0
    per_member = []
    for m in range(G):
        ms, cnt = (C.c_float * _lib.NUM_PASSES)(), C.c_int32()
        _lib.check(lib.meao_get_pass_times(pool.member_context(m), C.byref(ms), C.byref(cnt)))
        per_member.append(round(float(sum(ms)), 4))
        _lib.check(lib.meao_set_profiling(pool.member_context(m), 0))
    # validation of the timed (pipelined) path: every output checksummed, the first and last frame of every member vs the oracle
    host = [t.cpu().numpy() for t in out_dev]
    sums = [frame_checksum(a) for a in host]
    validated = mismatched = 0
    if args.validate_frames != 0:
        O, s = oracle_settings(w, h, cam, intensity, ao_format)
        for g in sorted({m for m in range(G)} | {n - 1 - m for m in range(G)}):
            want = O.run(frames[g], s, nthreads=O.host_cores(), result_only=True)["result"]
            validated += 1
            mismatched += int(not np.array_equal(host[g].view(want.dtype), want))
    paths = {f"member{m}->device{devices[0]}": ["same_device", "peer_direct", "staged"][pool.gather_path(m, devices[0])] for m in range(G)}
    pool.close()
    line = {
        "metric": "AO Mpixels/s (full multi-scale SSAO pipeline, depth resident in HBM)",
        "value": round(float(w) * h * n * steps / elapsed / 1e6, 1), "unit": "Mpixels/s",
        "n_gpus": len(set(devices)), "pool_members": G, "steps": steps, "steps_requested": args.steps, "warmup": args.warmup,
        "ms_per_step": round(elapsed / steps * 1e3, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32", "data": "synthetic",
        "config": {"workload": desc, "width": w, "height": h, "frames_per_step_per_member": B, "num_levels": 4,
                   "ao_storage": "R8" if ao_format == _lib.AO_R8 else "F16",
                   "host": "ONE process, meao_pool_* (C ABI): frame g -> member g mod G, one calling thread "
                           "(the pool enqueues each member's launches from its own worker thread)",
                   "member_devices": devices,
                   "downsample": "pipelined (meao_pool_prefetch_batch)" if pipelined else "own pass per step"},
        "per_member_ms": per_member, "gather_paths": paths,
        "validation": {"frames_checksummed": len(sums), "distinct_checksums": len(set(sums)),
                       "frames_vs_oracle": validated, "mismatching_frames": mismatched,
                       "validated_path": "the timed pipelined pool step"},
        "note": ("members share one device here: their kernels time-share, value is not a scaling number"
                 if len(set(devices)) < G else "one member per device"),
    }
    return line


def run_pool(args) -> int:
    print(json.dumps(measure_pool(args, args.pool)), flush=True)
    return 0


def measure_copy_ceiling(dev, nbytes=1 << 30, min_seconds=0.040):
    """What a plain device-to-device copy reaches on THIS box in THIS run: 1 GiB read + 1 GiB written per
    repetition (2 GiB working set, 8x the 256 MiB Infinity Cache), back-to-back repetitions for >= min_seconds after as
    long a warm-up, HIP events on torch's current stream.  Two forms, the faster one is the ceiling: Tensor.copy_ (the
    runtime's device copy) and an elementwise kernel (16 B per lane loads / stores)."""
    a = torch.full((nbytes // 4,), 1.0, dtype=torch.float32, device=dev)
    b = torch.empty_like(a)
    forms = {"Tensor.copy_": lambda: b.copy_(a), "elementwise_mul": lambda: torch.mul(a, 1.0, out=b)}
    out = {}
    for name, fn in forms.items():
        fn()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        reps = max(5, int(min_seconds / max(time.perf_counter() - t0, 1e-5)))
        for _ in range(reps):               # warm-up: clocks under a streaming load
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize(dev)
        out[name] = round(2.0 * nbytes * reps / (e0.elapsed_time(e1) * 1e-3) / 1e9, 1)
    del a, b
    best = max(out, key=out.get)
    return {"GBps": out[best], "method": best, "all_GBps": out, "bytes_per_repetition": 2 * nbytes,
            "note": "read + written bytes / HIP-event time; measured in this run on this box"}


def self_launch(args) -> int:
    """`python bench.py --gpus N` without a launcher: re-run this command line under torch.distributed.run, one rank
    per GPU, rendezvous on 127.0.0.1 at a free port -- exactly the command the driver issues for N > 1.  Rank 0's
    JSON line is this process's output.  RCCL needs one GPU per rank: with fewer visible devices the run is refused
    unless --dist-backend gloo (ranks then share devices; a functional check, not a scaling number)."""
    import subprocess
    ndev = torch.cuda.device_count()
    if ndev < args.gpus and args.dist_backend == "nccl":
        raise SystemExit(f"--gpus {args.gpus} but {ndev} visible device(s): RCCL needs one GPU per rank "
                         "(use --dist-backend gloo to let ranks share devices -- functional check only)")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(mdist.free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 1) // args.gpus)))
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")     # dmabuf IPC: what RCCL needs on this driver
    return subprocess.run(cmd, env=env).returncode


DUMP_LIMIT_BYTES = 64 * 10 ** 6     # --dump-outputs: all files of a run together stay below this
DUMP_SAMPLE_SEED = 0x5EED


def dump_outputs(path, outs, ao_format, rank, world):
    """--dump-outputs DIR: the AO frames `outs` (what the timed path wrote in its last step, one [H, W] device tensor per
    frame) as float32 AO values -- R8 storage decoded as code / 255, fp16 storage as its half value.  Frames that fit the
    budget are written whole: ao.npy [B, H, W].  Otherwise the same fixed, seeded sample of texel positions in every frame:
    ao_sample.npy [B, N] and ao_sample_index.npy [N] (flat index y * W + x, float64).  With N > 1 ranks every rank writes
    its own frames (file names end in _rank<r>) within 1/N of the budget."""
    os.makedirs(path, exist_ok=True)
    host = np.stack([t.cpu().numpy() for t in outs])
    ao = host.astype(np.float32) / np.float32(255) if ao_format == _lib.AO_R8 else host.view(np.float16).astype(np.float32)
    suffix = f"_rank{rank}" if world > 1 else ""
    budget = DUMP_LIMIT_BYTES // world - (1 << 16)          # headroom for the .npy headers
    B, h, w = ao.shape
    if ao.nbytes <= budget:
        np.save(os.path.join(path, f"ao{suffix}.npy"), ao)
        return {"dir": path, "files": [f"ao{suffix}.npy"], "frames": B, "texels_per_frame": h * w}
    n = min(h * w, budget // (4 * B + 8))
    index = np.sort(np.random.default_rng(DUMP_SAMPLE_SEED).choice(h * w, size=n, replace=False))
    np.save(os.path.join(path, f"ao_sample{suffix}.npy"), np.ascontiguousarray(ao.reshape(B, h * w)[:, index]))
    np.save(os.path.join(path, f"ao_sample_index{suffix}.npy"), index.astype(np.float64))
    return {"dir": path, "files": [f"ao_sample{suffix}.npy", f"ao_sample_index{suffix}.npy"], "frames": B,
            "texels_per_frame": int(n), "sample_seed": DUMP_SAMPLE_SEED}


def resolve_timed_region(steps, min_time_ms):
    """An explicit --steps is honoured exactly (the driver's contract: "time EXACTLY K steps"); only the flag-less default
    stretches the timed region to 100 ms.  --min-time-ms given explicitly always applies."""
    if min_time_ms is None:
        min_time_ms = 100.0 if steps is None else 0.0
    return (30 if steps is None else steps), min_time_ms


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None,
                    help="timed steps.  Given explicitly (the driver's contract) EXACTLY that many are timed, unless --min-time-ms is "
                         "given too; default 30, raised so that the timed region lasts 100 ms")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="4k")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the AO frames their last step computed to DIR/<name>.npy (float32; "
                         "a fixed, seeded sample of texels when the frames exceed 64 MB), for output-by-output comparison of builds")
    ap.add_argument("--batch", type=int, default=None,
                    help="independent frames per step per GPU (1..64); default: 133 Mpixels per step "
                         "(64 frames at 1080p, 16 at 4K, 4 at 8K)")
    ap.add_argument("--pool", type=int, default=0,
                    help="in-process host: ONE process drives this many pool members through meao_pool_* "
                         "(member m on device m mod visible devices); prints the same JSON incl. per_member_ms")
    ap.add_argument("--in-flight", type=int, default=1,
                    help="batches in flight: N contexts on N HIP streams, step k on stream k mod N "
                         "(lets the HBM-bound downsample of one batch overlap the VALU-bound passes of another)")
    ap.add_argument("--composite", action="store_true",
                    help="also time the next-tier composite kernel (AO x RGBA16F frame, Blit.shader pass 2); "
                         "reported separately, never part of `value`")
    ap.add_argument("--shaded", action="store_true",
                    help="next tier, reported separately: 'depth in -> shaded frame out' with the composite of each "
                         "step riding inside the next step's render kernel (meao_composite_enqueue), next to the "
                         "same work as separate composite launches")
    ap.add_argument("--ao-format", choices=["r8", "f16"], default=None,
                    help="override the AO storage of the workload (R8 = reference, F16 = fp16 AO)")
    ap.add_argument("--hq-levels", type=int, default=0,
                    help="variant (not the reference's wiring): the coarsest N levels also run Render.main "
                         "(wide) and the upsamples become main_premin*; changes config.workload")
    ap.add_argument("--exhaustive", action="store_true",
                    help="variant: SAMPLE_EXHAUSTIVELY (68 samples instead of 36); changes config.workload")
    ap.add_argument("--blend-tall-min-tiles", type=int, default=None, metavar="TILES",
                    help="meao_debug_set(MEAO_DEBUG_BLEND_TALL_MIN_TILES, TILES): L2 -> L1 blend launches of at least TILES 64x32 tiles use 64x64 tiles")
    ap.add_argument("--no-pipeline", action="store_true",
                    help="do not use meao_prefetch_batch: every step launches its own downsample pass instead of "
                         "carrying the next step's inside its last upsample kernel")
    ap.add_argument("--roctx", action="store_true",
                    help="meao_set_tracing: roctx ranges around every pass (for rocprofv3 --marker-trace)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-copy-ceiling", action="store_true",
                    help="skip the device-copy measurement (roofline.copy_ceiling_measured_GBps); fractions then use the guide's 6290 GB/s")
    ap.add_argument("--no-best-host-config", action="store_true",
                    help="skip the two-pool-members-on-one-device leg of the default N=1 line (best_host_config)")
    ap.add_argument("--no-other-workloads", action="store_true",
                    help="skip the short 1080p / 8K sub-measurements of the default N=1 line")
    ap.add_argument("--min-time-ms", type=float, default=None,
                    help="raise --steps so that the timed region lasts at least this long (clock state and rank skew "
                         "matter less in a >= 100 ms region); the JSON reports the steps actually timed; 0 = exactly --steps.  "
                         "Default: 100 when --steps is not given, 0 (exactly --steps) when it is")
    ap.add_argument("--validate-frames", type=int, default=-1,
                    help="frames per rank checked bit-for-bit against the CPU oracle after each timed region "
                         "(-1 = every frame at N=1, 2 per rank at N>1; 0 = checksums only)")
    ap.add_argument("--dist-backend", choices=["nccl", "gloo"], default="nccl",
                    help="process-group backend; nccl (= RCCL) is what a multi-GPU node uses.  gloo lets the N > 1 path of this "
                         "script run on a box with fewer GPUs than ranks (ranks then share devices: rank r on device r mod visible "
                         "devices) -- a functional check of sharding / fences / gathers / validation, not a scaling number")
    ap.add_argument("--launcher", action="store_true",
                    help="with --gpus 1: run through the self-launcher as well (torch.distributed.run, rendezvous on 127.0.0.1, a "
                         "one-rank process group of --dist-backend whose collectives carry fences / MAX / checksums): the driver's "
                         "N > 1 command path rehearsed on a 1-GPU box")
    ap.add_argument("--dry-run-topology", action="store_true",
                    help="print the rank -> device -> NUMA node -> CPU binding map `--gpus N` would use on this box (JSON) and exit; "
                         "nothing is launched")
    ap.add_argument("--no-numa-binding", action="store_true",
                    help="do not bind each rank's process to the CPUs of its GPU's NUMA node (default: bind where a node is known)")
    ap.add_argument("--skip-latency", action="store_true",
                    help="skip the single-frame latency loop (keeps profiler traces to the batched launches)")
    args = ap.parse_args()
    args.steps, args.min_time_ms = resolve_timed_region(args.steps, args.min_time_ms)

    if args.dry_run_topology:
        ndev = torch.cuda.device_count() if torch.cuda.is_available() else 0
        print(json.dumps({"ranks": args.gpus, "visible_devices": ndev, "map": topology.dry_run(args.gpus, ndev)}), flush=True)
        return 0
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (there is no CPU fallback for the product path)")
    if args.pool > 0:
        if args.dump_outputs:
            raise SystemExit("--dump-outputs writes the outputs of the single-context timed path; it does not apply to --pool")
        return run_pool(args)

    if (args.gpus > 1 or args.launcher) and "WORLD_SIZE" not in os.environ:
        return self_launch(args)                # plain `python bench.py --gpus N`: become the launcher of N ranks

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")

    ndev = torch.cuda.device_count()
    if local_rank >= ndev and args.dist_backend == "nccl":
        raise SystemExit(f"LOCAL_RANK {local_rank} but {ndev} visible device(s): RCCL needs one GPU per rank (--dist-backend gloo shares devices)")
    local_rank = local_rank % ndev                               # only ever wraps with --dist-backend gloo
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    # host placement: this rank's process on the socket its GPU hangs off (miniengineao_amd.topology; no-op where no node is known)
    placement = topology.bind_rank(local_rank, rank) if not args.no_numa_binding else {"rank": rank, "device": local_rank, "bound": False,
                                                                                      "action": "--no-numa-binding"}
    mdist.init(args.dist_backend, dev)                           # nccl == RCCL on ROCm

    wl = Workload(args.workload, args, dev, local_rank, rank, world, batch=args.batch, in_flight=args.in_flight)
    w, h, B, ao, ao_format, cam, intensity = wl.w, wl.h, wl.B, wl.ao, wl.ao_format, wl.cam, wl.intensity
    pipelined = wl.pipelined
    n_validate = args.validate_frames if args.validate_frames >= 0 else (B if world == 1 else 2)

    steps_requested = args.steps
    wl.ramp(0.250)          # (80 ms until round 5: with the driver's 20 timed steps = 11 ms the region still sat on the slope, render 178 vs 169 us)
    args.steps = wl.steps_for(args.min_time_ms, args.steps)
    elapsed, my_elapsed, pass_ms, samples = wl.timed(args.steps, args.warmup)
    per_rank_ms = mdist.gather_floats(my_elapsed / args.steps * 1e3, dev)
    rank_nodes = mdist.gather_floats(float(-2 if placement.get("numa_node") is None else placement["numa_node"]), dev)
    rank_bound = mdist.gather_floats(float(bool(placement.get("bound"))), dev)
    # physical devices behind the ranks (one node: the device index identifies the GPU); < world only with --dist-backend gloo
    n_devices = len({int(d) for d in mdist.gather_floats(float(local_rank), dev)})

    # ---- validation of the TIMED path, right behind its timed region: what out_dev holds now was written by the
    # last step of that region (prefetched downsample consumed, final pass = the fused kernel)
    check_timed, sums_timed = wl.validate(n_validate)
    dumped = dump_outputs(args.dump_outputs, wl.last_outputs(), ao_format, rank, world) if args.dump_outputs else None

    # A timed region shorter than 50 ms (the driver's --steps 20 = 10 ms) carries its own long-form cross-check: the same step
    # timed over >= 100 ms right behind it (after the validation's idle gap: clocks ramped again).  Outside `value`.
    long_form = None
    if elapsed < 0.050:
        wl.ramp(0.100)
        long_steps = wl.steps_for(100.0, args.steps)
        l_elapsed, _, _, _ = wl.timed(long_steps, 3)
        long_form = {"value_long": round(float(w) * h * B * long_steps * world / l_elapsed / 1e6, 1),
                     "ms_per_step_long": round(l_elapsed / long_steps * 1e3, 4), "steps_long": long_steps,
                     "note": "the same pipelined step, per-pass events on, timed over >= 100 ms right after the headline region "
                             "(which lasted < 50 ms); not part of `value`"}

    # The same K steps once more WITHOUT the per-pass HIP events (two event records per launch = eight marker packets per step
    # on the stream): what the library does for a host that does not profile it.  `value` stays on the timed region above, whose
    # events the roofline rows come from; this leg says what those events cost.
    wl.ramp(0.100)          # (the validation above left the device idle: back to steady clocks first, as before the main region)
    ne_elapsed, _, _, _ = wl.timed(args.steps, 3, pass_events=False)
    without_events = {"value": round(float(w) * h * B * args.steps * world / ne_elapsed / 1e6, 1),
                      "ms_per_step": round(ne_elapsed / args.steps * 1e3, 4),
                      "note": "the timed path with meao_set_profiling off: no event records between the launches"}
    # ... and with the event pair of the dominant kernel alone (MEAO_DEBUG_PROFILE_PASS_MASK): what a host pays that wants that one
    # duration in a throughput run.  Its bracket opens right behind the previous kernel, so it holds the dispatch gap as well
    # (a few us more than the same kernel between the markers of its neighbours, which is what rocprofv3's kernel trace agrees with).
    dominant_slot = int(np.argmax(pass_ms))
    do_elapsed, _, do_pass_ms, _ = wl.timed(args.steps, 3, pass_mask=1 << dominant_slot)
    dominant_events_only = {"value": round(float(w) * h * B * args.steps * world / do_elapsed / 1e6, 1),
                            "ms_per_step": round(do_elapsed / args.steps * 1e3, 4),
                            "kernel": _lib.PASS_NAMES[dominant_slot], "launch_ms": round(do_pass_ms[dominant_slot], 5),
                            "note": "the timed path with one event pair per step instead of eight"}

    # for reference, the same K steps as the plain launch sequence (every step runs its own downsample
    # pass), with per-pass events: this is where the north-star sub-path (render + upsample passes,
    # nothing else inside those kernels) is timed
    plain, plain_pass_ms, check_plain, sums_plain = None, None, None, None
    if pipelined:
        wl.use_prefetch = False
        wl.ramp(0.100)      # steady clocks for this leg too: with an explicit small --steps it would otherwise be timed on the ramp
        plain_elapsed, _, plain_pass_ms, _ = wl.timed(args.steps, 3)
        plain = {"value": round(float(w) * h * B * args.steps * world / plain_elapsed / 1e6, 1),
                 "ms_per_step": round(plain_elapsed / args.steps * 1e3, 4),
                 "pass_ms": {n: round(plain_pass_ms[k], 5) for k, n in enumerate(_lib.PASS_NAMES) if plain_pass_ms[k] > 0}}
        check_plain, sums_plain = wl.validate(min(n_validate, 2))
        wl.use_prefetch = True
    else:
        plain_pass_ms = pass_ms

    validation = {"timed_path": "pipelined (meao_prefetch_batch + fused last kernel)" if pipelined else "plain launch sequence",
                  "pipelined" if pipelined else "plain": check_timed,
                  "frames_checksummed": check_timed["frames_checksummed"], "distinct_checksums": check_timed["distinct_checksums"],
                  "frames_vs_oracle": check_timed["frames_vs_oracle"] + (check_plain["frames_vs_oracle"] if check_plain else 0),
                  "mismatching_frames": check_timed["mismatching_frames"] + (check_plain["mismatching_frames"] if check_plain else 0),
                  "sharding": "frame g -> rank g mod world (frames_for_rank)",
                  "rank0_first_checksum": sums_timed[0][0] if sums_timed and sums_timed[0] else None}
    if check_plain is not None:
        validation["plain"] = check_plain
        validation["pipelined_equals_plain_all_frames"] = sums_timed == sums_plain

    # the box's own streaming ceiling, measured in this run (rank 0's device; every rank runs it so that nobody idles)
    copy_ceiling = measure_copy_ceiling(dev) if not args.no_copy_ceiling else None
    ceiling_gbps = copy_ceiling["GBps"] if copy_ceiling else HBM_COPY_CEILING_GBPS

    total_pixels = float(w) * h * B * args.steps * world
    value = total_pixels / elapsed / 1e6
    step_ms = elapsed / args.steps * 1e3

    # roofline of the dominant kernel: algorithmic bytes per launch / measured launch duration
    passes, alg, names = pass_table(ao, pass_ms, B, pipelined, args.workload, ceiling_gbps)
    ren_ups_bytes = sum(ao.algorithmic_bytes()[1:])    # render + upsample passes only (north_star's sub-path)
    dominant = int(np.argmax(pass_ms))
    dom_gbps = alg[dominant] * B / (pass_ms[dominant] * 1e-3) / 1e9
    traffic = pmc_traffic(args.workload, names[dominant], B)
    kernel_ms = float(sum(pass_ms))
    whole_gbps = sum(alg) * B / (step_ms * 1e-3) / 1e9          # all algorithmic bytes of a step / the STEP time (gaps included)
    # north_star's sub-path: the render + upsample passes alone (plain launch sequence: nothing else rides in those kernels)
    ren_ups_ms = sum(plain_pass_ms[1:])
    ren_ups_gbps = ren_ups_bytes * B / (ren_ups_ms * 1e-3) / 1e9
    # ... and the same sub-path against the VALU issue roof: committed SQ_INSTS_VALU of its launches (plain sequence) / their time
    plain_rows, _, _ = pass_table(ao, plain_pass_ms, B, False, args.workload, ceiling_gbps)
    sub_rows = [r for r in plain_rows if r["kernel"] != "downsample"]
    sub_valu = None
    if sub_rows and all(r["valu_frac"] is not None for r in sub_rows):
        sub_valu = round(sum(r["valu_frac"] * r["ms"] for r in sub_rows) / sum(r["ms"] for r in sub_rows), 4)
    dom_limits = limiter_fields(traffic, pass_ms[dominant], ceiling_gbps)
    roofline = {"bound": "hbm",
                # which roof the dominant kernel is nearer to: moved bytes / the copy ceiling of this run vs VALU wave-instructions / the
                # VALU issue roof (both from the committed PMC passes of this build; None when those belong to another build)
                "limiter": dom_limits["limiter"], "valu_frac": dom_limits["valu_frac"],
                "valu_peak_wave_insts_per_s": VALU_PEAK_WAVE_INSTS_PER_S,
                "valu_clock": "2.4 GHz spec clock (the PMC passes' GRBM_GUI_ACTIVE implies ~2.3 GHz under load: fractions are lower bounds)",
                "kernel": names[dominant], "achieved": round(dom_gbps, 1),
                "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": round(dom_gbps / HBM_PEAK_GBPS, 4),
                "traffic": traffic, "launch_ms": round(pass_ms[dominant], 5), "event_samples": samples,
                "event_period": PASS_EVENT_PERIOD,      # HIP events around the launches of every step of the timed region
                "whole_frame": {"GBps": round(whole_gbps, 1), "frac": round(whole_gbps / HBM_PEAK_GBPS, 4),
                                "over": "ms_per_step (launch gaps included)"},
                # north_star's sub-path (target: frac >= 0.60), timed per pass in the plain launch sequence
                "render_plus_upsample": {"GBps": round(ren_ups_gbps, 1), "frac": round(ren_ups_gbps / HBM_PEAK_GBPS, 4),
                                         "ms_per_launch": round(ren_ups_ms, 5),
                                         "algorithmic_MB": round(ren_ups_bytes * B / 1e6, 2),
                                         "timed_in": "plain_launch_sequence (same process, per-pass HIP events)",
                                         "valu_frac": sub_valu,
                                         "valu_floor_as_frac_of_hbm_roofline": SUBPATH_VALU_FLOOR_FRAC_OF_HBM_ROOFLINE,
                                         "reading": "the sub-path is VALU-bound: `frac` of the HBM roofline, `valu_frac` of the VALU issue "
                                                    "roof; with its bit-exact instruction mix issuing at the measured best rate and nothing "
                                                    "ever waiting it would reach `valu_floor_as_frac_of_hbm_roofline` of the HBM roofline",
                                         "passes": sub_rows},
                # the same fraction in bytes that actually moved (committed PMC traffic of the dominant kernel / its time in THIS run)
                "real_traffic_frac": None if traffic_bytes(traffic) is None else round(
                    traffic_bytes(traffic) / (pass_ms[dominant] * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4),
                # against what a plain copy reaches on this box in this run (guide figure 6290 GB/s only with --no-copy-ceiling)
                "copy_ceiling_measured_GBps": copy_ceiling["GBps"] if copy_ceiling else None,
                "copy_ceiling": copy_ceiling,
                "vs_copy_ceiling_frac": round(dom_gbps / ceiling_gbps, 4),
                "real_traffic_vs_copy_ceiling_frac": dom_limits["moved_bytes_vs_copy_ceiling"],
                "passes": passes}

    cpu = None
    if rank == 0 and world == 1 and not args.no_cpu_baseline and not (args.hq_levels or args.exhaustive):
        cpu = cpu_baseline(w, h, cam, intensity, ao_format, wl.frames[0])

    stream, dptr, optr = wl.streams[0], wl.dptr, wl.optrs[0]
    composite = None
    if args.composite:
        # next-tier consumer of the AO texture: color.rgba *= ao, 17 bytes per texel, HBM-bound
        colors = [torch.ones((h, w, 4), dtype=torch.float16, device=dev) for _ in range(B)]
        reps = 10
        for f in range(B):
            ao.composite_device(_lib.COMPOSITE_MULTIPLY, optr[f], colors[f].data_ptr(), 0, stream)
        wl.fence()
        tc = time.perf_counter()
        for _ in range(reps):
            for f in range(B):
                ao.composite_device(_lib.COMPOSITE_MULTIPLY, optr[f], colors[f].data_ptr(), 0, stream)
        torch.cuda.synchronize(dev)
        per_frame_ms = (time.perf_counter() - tc) * 1e3 / (reps * B)    # back-to-back launches, device-synchronised wall time
        cbytes = w * h * (16 + (1 if ao_format == _lib.AO_R8 else 2))
        cg = cbytes / (per_frame_ms * 1e-3) / 1e9
        composite = {"kernel": "composite_multiply", "ms_per_frame": round(per_frame_ms, 5),
                     "algorithmic_MB_per_frame": round(cbytes / 1e6, 2), "GBps": round(cg, 1),
                     "frac": round(cg / HBM_PEAK_GBPS, 4), "bound": "hbm"}

    shaded = None
    if args.shaded:
        # depth in -> shaded frame out: every step = AO of B frames + composite (color.rgba *= ao) of those frames
        colors = [torch.ones((h, w, 4), dtype=torch.float16, device=dev) for _ in range(B)]
        cptr = [t.data_ptr() for t in colors]

        def shaded_steps(pipelined_composite):
            for _ in range(args.steps):
                if pipelined:
                    ao.prefetch_device(dptr)
                ao.execute_device(dptr, optr, stream)          # carries the composite enqueued by the previous step
                if pipelined_composite:
                    ao.composite_enqueue_device(_lib.COMPOSITE_MULTIPLY, optr, cptr)
                else:
                    for f in range(B):
                        ao.composite_device(_lib.COMPOSITE_MULTIPLY, optr[f], cptr[f], 0, stream)
            ao.composite_flush(stream)
        shaded = {}
        for name, flag in (("separate_composite_launches", False), ("composite_inside_next_render", True)):
            shaded_steps(flag)                                  # warm-up
            wl.fence()
            ts = time.perf_counter()
            shaded_steps(flag)
            wl.fence()
            dt = mdist.max_over_ranks(time.perf_counter() - ts, dev)
            shaded[name] = {"Mpixels_per_s": round(float(w) * h * B * args.steps * world / dt / 1e6, 1),
                            "ms_per_step": round(dt / args.steps * 1e3, 4)}
        shaded["note"] = "next tier, not part of `value`: AO + Blit.shader pass 2 on an RGBA16F frame per step"

    # single-frame use (one frame per call, the real-time case): back-to-back calls, and call + wait per frame
    latency_ms, single = None, None
    if not args.skip_latency:
        def one_frame_ctx(**kw):
            c = AmbientOcclusion(w, h, device=local_rank, num_levels=4, ao_format=ao_format, max_batch=1,
                                 near_clip=cam.near, far_clip=cam.far, projection00=cam.proj00(w, h),
                                 reversed_z=cam.reversed_z, hq_levels=args.hq_levels,
                                 sample_set=_lib.SAMPLES_EXHAUSTIVE if args.exhaustive else _lib.SAMPLES_CHECKER, **kw)
            c.intensity = intensity
            return c
        lat_iters = 50
        single = {}
        # what the validated batched run left in frame 0: every one-frame variant below must reproduce it (same depth frame)
        frame0_validated = wl.out_dev[0][0].clone()
        single_mismatches = {}
        # "pipelined": a stream of single frames whose next depth buffer is known one call ahead
        # (meao_prefetch_batch with n = 1: each call's last kernel carries the next frame's downsample pass).
        # "direct" = the library's default sequence (downsample | render | blends | final)
        variants = (("direct", {}), ("direct_pipelined", {"pipelined": True}))
        for name, kw in variants:
            kw = dict(kw)
            debug = kw.pop("_debug", {})
            c = one_frame_ctx(**kw)
            for debug_key, debug_value in debug.items():
                c.debug_set(debug_key, debug_value)
            for sync_each in (False, True):
                for _ in range(3):
                    if name == "direct_pipelined":
                        c.prefetch_device(dptr[:1])
                    c.execute_device(dptr[:1], optr[:1], stream)
                wl.fence()
                t0 = time.perf_counter()
                for _ in range(lat_iters):
                    if name == "direct_pipelined":
                        c.prefetch_device(dptr[:1])
                    c.execute_device(dptr[:1], optr[:1], stream)
                    if sync_each:
                        torch.cuda.synchronize(dev)
                torch.cuda.synchronize(dev)
                single[name + ("_call_and_wait_ms" if sync_each else "_back_to_back_ms")] = \
                    round((time.perf_counter() - t0) / lat_iters * 1e3, 4)
            single_mismatches[name] = int((wl.out_dev[0][0] != frame0_validated).sum().item())
            c.close()
        single["texels_differing_from_the_validated_batched_result"] = single_mismatches
        if any(single_mismatches.values()):
            raise SystemExit(f"one-frame-per-call results differ from the validated batched result: {single_mismatches}")
        latency_ms = single["direct_back_to_back_ms"]

    desc, nfl = wl.desc, wl.nfl
    wl.close()
    del wl

    # BASELINE configs 2 and 5 on the same clock: short sub-measurements (N = 1, default line only)
    others = None
    if rank == 0 and world == 1 and not args.no_other_workloads and not (args.hq_levels or args.exhaustive):
        others = {}
        for name in ("1080p", "8k"):
            if name != args.workload:
                torch.cuda.empty_cache()
                others[name] = measure_other_workload(name, args, dev, local_rank, ceiling_gbps)

    # The best VALIDATED host configuration on one device, measured in the same run: the step's frames dealt
    # to two pool members (meao_pool_*), whose launch tails and heads overlap.  `value` / `roofline` stay on the single
    # context above, where per-kernel durations are attributable.
    best_host = None
    if (rank == 0 and world == 1 and not args.no_best_host_config and B >= 2 and nfl == 1 and pipelined
            and not (args.hq_levels or args.exhaustive or args.ao_format)):
        torch.cuda.empty_cache()
        # the step dealt to two pool members on device 0, validated like the headline (every output checksummed, first / last
        # frame of every member vs the oracle)
        tried = []
        for members in (2,):
            pl = measure_pool(args, members, B // members, ramp_s=0.050)
            tried.append({"pool_members": members, "frames_per_member": B // members,
                          "value": pl["value"], "ms_per_step": pl["ms_per_step"], "steps": pl["steps"],
                          "per_member_ms": pl["per_member_ms"], "validation": pl["validation"]})
        ok = [t for t in tried if t["validation"]["mismatching_frames"] == 0 and t["validation"]["frames_vs_oracle"] > 0]
        if ok:
            best = max(ok, key=lambda t: t["value"])
            best_host = dict(best, unit="Mpixels/s", vs_single_context=round(best["value"] / value, 4),
                             host="ONE process, meao_pool_* members on device 0 (frame g -> member g mod members), pipelined step",
                             candidates=[{k: t[k] for k in ("pool_members", "value", "ms_per_step")} for t in tried],
                             note="kernels of co-running members overlap: per-kernel durations are not "
                                  "attributable there, so `value` and the roofline rows stay on the single-context leg")

    if rank == 0:
        line = {
            "metric": "AO Mpixels/s (full multi-scale SSAO pipeline, depth resident in HBM)",
            "value": round(value, 1), "unit": "Mpixels/s", "n_gpus": n_devices, "ranks": world,
            "devices_shared": n_devices < world, "steps": args.steps, "steps_requested": steps_requested,
            "steps_note": None if args.steps == steps_requested else
                f"--min-time-ms {args.min_time_ms:g} raised the timed region from {steps_requested} to {args.steps} steps",
            "warmup": args.warmup, "ms_per_step": round(step_ms, 4),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32",
            "data": "synthetic",
            "config": {"workload": desc, "width": w, "height": h, "frames_per_step_per_gpu": B,
                       "num_levels": 4, "ao_storage": "R8" if ao_format == _lib.AO_R8 else "F16",
                       "numerics": "strict (bit-exact vs CPU oracle)",
                       "sharding": f"frames x{world}", "batches_in_flight": nfl, "process_group": args.dist_backend if mdist.group_info()["initialized"] else None,
                       "downsample": ("own pass per step" if not pipelined else
                                      "pipelined: each step's last kernel carries the next step's downsample pass (meao_prefetch_batch)")},
            "roofline": roofline, "cpu_baseline": cpu, "composite_next_tier": composite,
            "depth_in_to_shaded_frame_out": shaded,
            "per_rank_ms_per_step": [round(x, 4) for x in per_rank_ms],
            # rank -> device -> NUMA node of the device -> was the rank's process bound to that node's CPUs (rank 0's record in full)
            "topology": {"rank0": placement,
                         "ranks": [{"rank": r, "numa_node": None if n < -1 else int(n), "bound": bool(b)}
                                   for r, (n, b) in enumerate(zip(rank_nodes, rank_bound))]},
            "world_seen_by_process_group": mdist.world_size(),
            "world_seen_by_rccl": mdist.world_size() if (world == 1 or args.dist_backend == "nccl") else None,
            # what the collectives of this run actually went through (world_seen_by_rccl is 1 with no group at all, too)
            "process_group_in_use": mdist.group_info(),
            "validation": validation,
            "single_frame_latency_ms": None if latency_ms is None else round(latency_ms, 4),
            "single_frame": single,
            "value_long": None if long_form is None else long_form["value_long"],
            "ms_per_step_long": None if long_form is None else long_form["ms_per_step_long"],
            "long_form_cross_check": long_form,
            "plain_launch_sequence": plain,
            "without_pass_events": without_events,
            "with_dominant_kernel_events_only": dominant_events_only,
            "sum_kernel_ms_per_step": round(kernel_ms, 4),
            "other_workloads": others,
            "best_host_config": best_host,
        }
        if dumped is not None:
            line["dumped_outputs"] = dumped
        # the headline must be what the clock says: pixels of the timed region / its duration (round 5: a loop variable named
        # `value` once overwrote it between here and its computation -- caught by reading the line, now caught by the script)
        implied = float(w) * h * B * world / (line["ms_per_step"] * 1e-3) / 1e6
        if abs(line["value"] - implied) > 0.002 * implied:
            raise SystemExit(f"bench.py: value {line['value']} disagrees with pixels / ms_per_step = {implied:.1f}")
        print(json.dumps(line), flush=True)
    mdist.shutdown()
    return 0


if __name__ == "__main__":
    sys.exit(main())
