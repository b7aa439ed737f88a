"""Long randomized GPU-vs-oracle sweep (not part of the default suite; run on demand):
    python tools/fuzz_gpu.py [count] [seed0]
    python tools/fuzz_gpu.py --sequences N [seed0]     N call sequences with fresh seeds, one long-lived context (or pool) each
Emphasises the vector fast paths (widths that are multiples of 4 / 8 / 64) and tile-edge cases; a quarter of the cases draw
their upsample or noise-filter tolerance outside the exact-division range (the IEEE-division column of RTZ contexts)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from miniengineao_amd import synth  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import helpers as H  # noqa: E402


def run_sequences(count, seed0):
    """The generator and model of tests/call_model.py with fresh seeds, driven by the stepped Driver of
    tests/test_call_sequences_gpu.py: every case of the suite's stepped and pool modes in turn -- those that draw reservations, resizes
    and sized announcements (tests/test_dynamic_resolution_sequences_gpu.py) and those that draw mixed-size batches into them
    (tests/test_mixed_size_sequences_gpu.py) included -- and both forms of the carried pass."""
    import pytest
    from miniengineao_amd import _lib as L
    from tests import call_model as M
    from tests.test_call_sequences_gpu import Driver          # the call-sequence driver stays in its suite
    from tests.linear_depth import linearize
    O.build()
    lin_c = linearize()
    cases = [("stepped", n) for n in sorted(M.CASES)] + [("pool_stepped", n) for n in sorted(M.POOL_CASES)]
    cases += [("dyn_stepped", n) for n in sorted(M.DYN_CASES)] + [("dyn_pool_stepped", n) for n in sorted(M.DYN_POOL_CASES)]
    cases += [("mix_stepped", n) for n in sorted(M.MIX_CASES)] + [("mix_pool_stepped", n) for n in sorted(M.MIX_POOL_CASES)]
    bad = 0
    for k in range(count):
        kind, name = cases[k % len(cases)]
        seed, own_launch = seed0 + k, (k // len(cases)) % 2
        cfg, prof, _ = M.case_profile(kind, name)
        kw = dict(linear=cfg.get("linear", False), rtz=cfg.get("rtz", True), pipelined=cfg.get("pipelined", True))
        pal = M.palette(kw["linear"])
        ops = M.generate(seed, prof, pal, pal[0], **kw)
        model = M.fresh_model(prof, cfg)
        d = Driver(O, cfg, prof, own_launch, lin_c, stepped=True, seed=seed)
        try:
            d.run(ops, model)
        except (AssertionError, L.MeaoError, pytest.fail.Exception) as e:     # (pytest.raises that did not raise is no AssertionError)
            bad += 1
            print("MISMATCH sequence", kind, name, "seed", seed, "own_launch", own_launch, str(e)[:600], flush=True)
        finally:
            d.close()
    print(f"fuzz: {count} sequences, {bad} failing")
    return bad


if "--sequences" in sys.argv:
    at = sys.argv.index("--sequences")
    sys.exit(1 if run_sequences(int(sys.argv[at + 1]), int(sys.argv[at + 2]) if len(sys.argv) > at + 2 else 7000) else 0)

count = int(sys.argv[1]) if len(sys.argv) > 1 else 200
seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 5000
from miniengineao_amd import _lib, codehash  # noqa: E402
print("library", os.path.relpath(_lib.LIB_PATH, ROOT), "device code sha256", codehash.device_code_sha256(_lib.LIB_PATH), flush=True)
bad = 0
for k in range(count):
    rng = np.random.default_rng(seed0 + k)
    mode = k % 4
    if mode == 0:
        w, h = int(rng.integers(1, 200)) * 4, int(rng.integers(1, 400))
    elif mode == 1:
        w, h = int(rng.integers(1, 14)) * 64 + int(rng.choice([0, 4, 8, 60])), int(rng.integers(1, 10)) * 32 + int(rng.integers(0, 3))
    elif mode == 2:
        w, h = int(rng.integers(1, 900)), int(rng.integers(1, 500))
    else:
        w, h = int(rng.integers(30, 90)) * 8, int(rng.integers(20, 60)) * 8
    reversed_z = bool(rng.integers(0, 2))
    cam = synth.Camera(near=float(rng.uniform(0.01, 0.6)), far=float(rng.uniform(10, 2000)),
                       fov_y_deg=float(rng.uniform(12, 90)), reversed_z=reversed_z)
    depth_format = int(rng.integers(0, 4))
    s = H.settings(O, w, h, cam=cam, ao_format=int(rng.integers(0, 2)), f16_rounding=int(rng.integers(0, 2)),
                   num_levels=int(rng.integers(1, 5)), noise_filter_tolerance=float(rng.uniform(-8, 0)),
                   blur_tolerance=float(rng.uniform(-8, -1)), upsample_tolerance=float(rng.uniform(-12, -1)),
                   thickness_modifier=float(rng.uniform(1, 10)), intensity=float(rng.uniform(0, 2)),
                   depth_format=depth_format)
    if k % 8 in (1, 6):     # a quarter of the cases: tolerances outside the exact-division range (RTZ contexts run DIV = 1)
        which = int(rng.integers(0, 3))
        if which == 0:
            s.upsample_tolerance = float(rng.uniform(-46, -13.25))
        elif which == 1:
            s.upsample_tolerance = float(rng.uniform(6.03, 40))
        else:
            s.noise_filter_tolerance = float(rng.uniform(9.04, 40))
    if k % 2:
        s.hq_levels, s.sample_set = int(rng.integers(0, s.num_levels + 1)), int(rng.integers(0, 2))
        s.single_pass_stereo = bool(rng.integers(0, 2))
    raw = synth.occluder_field(w, h, seed=k, n_rects=20, n_discs=20, cam=cam)
    if k % 3 == 0:
        x0, y0 = int(rng.integers(0, w)), int(rng.integers(0, h))
        raw[y0:y0 + 50, x0:x0 + 70] = 0.0 if reversed_z else 1.0
    hostile = depth_format == 0 and k % 5 == 0
    if hostile:      # NaN / inf / negative / > 1 / denormal raw depths sprinkled in (IEEE-division bodies)
        bad_px = H.hostile_frame(w, h, seed0 + k, cam=cam, density=0.003)
        mask = rng.random((h, w)) < 0.004
        raw = np.where(mask, bad_px, raw).astype(np.float32)
    depth = O.encode_depth(raw, depth_format) if not hostile else raw
    want = O.run(depth, s, nthreads=8)
    same = (lambda a, b: H.nan_aware_equal(a, b)[0]) if hostile or k % 8 in (1, 6) else np.array_equal
    from miniengineao_amd import AmbientOcclusion
    ao = AmbientOcclusion(w, h, num_levels=s.num_levels, ao_format=s.ao_format, f16_rounding=s.f16_rounding,
                          depth_format=depth_format, near_clip=s.near_clip, far_clip=s.far_clip,
                          projection00=s.proj00, reversed_z=reversed_z, max_batch=2, hq_levels=s.hq_levels,
                          sample_set=s.sample_set, single_pass_stereo=s.single_pass_stereo,
                          pipelined=bool(k % 2))
    ao.noiseFilterTolerance, ao.blurTolerance, ao.upsampleTolerance = s.noise_filter_tolerance, s.blur_tolerance, s.upsample_tolerance
    ao.thicknessModifier, ao.intensity = s.thickness_modifier, s.intensity
    if k % 7 == 3:          # a seventh of the cases: the L2 -> L1 pass on 64 x 64 tiles whatever the size (large R8 batches take them by default)
        from miniengineao_amd import _lib
        ao.debug_set(_lib.DEBUG_BLEND_TALL_MIN_TILES, 1)
        ao.debug_set(_lib.DEBUG_NESTED_MAX_TILES, 0)
    if k % 5 == 2:          # a fifth: the full-resolution pass on 64 x 64 tiles whatever the size (calls with many tiles take them by default)
        from miniengineao_amd import _lib
        ao.debug_set(_lib.DEBUG_FINAL_SMALL_MAX_TILES, 0)
    outs = ao.render_batch([depth, depth])
    ok = same(outs[0], want["result"]) and same(outs[1], want["result"])
    for i in H.valid_debug_ids(s.num_levels, s.hq_levels):
        ok = ok and same(ao.debug_buffer(i, frame=1), want[H.NAMES[i]])
    if k % 3 == 1:
        # the pipelined path: announce the same frames, run twice; the second call consumes the downsample
        # that rode inside the first call's last kernel
        import torch
        raw_bytes = np.ascontiguousarray(depth).view(np.uint8)
        d_in = [torch.from_numpy(raw_bytes.copy()).cuda() for _ in range(2)]
        d_out = [torch.zeros((h, w), dtype=torch.uint8 if s.ao_format == 0 else torch.int16, device="cuda") for _ in range(2)]
        pin, pout = [t.data_ptr() for t in d_in], [t.data_ptr() for t in d_out]
        ao.prefetch_device(pin)
        ao.execute_device(pin, pout)
        ao.execute_device(pin, pout)
        ao.synchronize()
        for t in d_out:
            ok = ok and same(t.cpu().numpy().view(want["result"].dtype), want["result"])
        for i in H.valid_debug_ids(s.num_levels, s.hq_levels):
            ok = ok and same(ao.debug_buffer(i, frame=1), want[H.NAMES[i]])
    ao.close()
    if not ok:
        bad += 1
        print("MISMATCH case", k, "seed", seed0 + k, (w, h), s)
print(f"fuzz: {count} cases, {bad} mismatching")
sys.exit(1 if bad else 0)
