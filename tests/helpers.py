"""Shared helpers of the parity tests: one Settings object drives both the oracle and the
C-ABI library so that every comparison runs on identical inputs and parameters."""
from __future__ import annotations

import dataclasses

import numpy as np

from miniengineao_amd import synth

NAMES = {1: "linear_depth", 2: "low_depth1", 3: "low_depth2", 4: "low_depth3", 5: "low_depth4",
         6: "tiled_depth1", 7: "tiled_depth2", 8: "tiled_depth3", 9: "tiled_depth4",
         10: "occlusion1", 11: "occlusion2", 12: "occlusion3", 13: "occlusion4",
         14: "combined1", 15: "combined2", 16: "combined3", 17: "result",
         18: "occlusion_hq1", 19: "occlusion_hq2", 20: "occlusion_hq3", 21: "occlusion_hq4"}


def settings(O, w, h, cam=synth.DEFAULT_CAMERA, **kw):
    return O.Settings(w, h, proj00=cam.proj00(w, h), near_clip=cam.near, far_clip=cam.far,
                      reversed_z=cam.reversed_z, **kw)


def component(s, max_batch=1, device=0, debug=None, **kw):
    """AmbientOcclusion (C ABI) configured exactly like oracle Settings ``s``.  ``debug``: {meao_debug_key: value}
    launch-structure overrides applied through meao_debug_set."""
    from miniengineao_amd import AmbientOcclusion
    ao = AmbientOcclusion(s.width, s.height, device=device, num_levels=s.num_levels,
                          ao_format=s.ao_format, f16_rounding=s.f16_rounding, max_batch=max_batch,
                          near_clip=s.near_clip, far_clip=s.far_clip, projection00=s.proj00,
                          reversed_z=s.reversed_z, hq_levels=s.hq_levels, sample_set=s.sample_set,
                          single_pass_stereo=s.single_pass_stereo, **kw)
    ao.noiseFilterTolerance = s.noise_filter_tolerance
    ao.blurTolerance = s.blur_tolerance
    ao.upsampleTolerance = s.upsample_tolerance
    ao.thicknessModifier = s.thickness_modifier
    ao.intensity = s.intensity
    for key, value in (debug or {}).items():
        ao.debug_set(key, value)
    return ao


def valid_debug_ids(num_levels, hq_levels=0):
    ids = list(range(1, 10))
    ids += [10 + k for k in range(num_levels)]
    ids += [14 + k for k in range(num_levels - 1)]
    ids.append(17)
    ids += [17 + k for k in range(1, num_levels + 1) if k > num_levels - hq_levels]
    return ids


def diff_report(name, got, want):
    bad = np.argwhere(got != want)
    first = tuple(bad[0])
    return (f"{name}: {len(bad)} of {got.size} texels differ; first at {first}: "
            f"got {got[first]!r} want {want[first]!r}")


def compare(got, want, what):
    ok, _ = nan_aware_equal(got, want)
    assert ok, diff_report(what, got, want)


def same(got, want, what):
    assert np.array_equal(got, want), diff_report(what, got, want)


# ---- small things the GPU suites share

PASS_DOWNSAMPLE = 0                  # meao_pass launch slot
DEPTH_FORMATS = {"f32": 0, "unorm16": 1, "unorm24": 2, "f16": 3}

# FrameParams field -> oracle Settings field
ORACLE_FIELD = {"nearClipPlane": "near_clip", "farClipPlane": "far_clip", "projection00": "proj00",
                "usesReversedZBuffer": "reversed_z", "singlePassStereoEnabled": "single_pass_stereo",
                "intensity": "intensity", "thicknessModifier": "thickness_modifier",
                "noiseFilterTolerance": "noise_filter_tolerance", "blurTolerance": "blur_tolerance",
                "upsampleTolerance": "upsample_tolerance"}


def frame_settings(base, fp):
    """oracle Settings of one frame: `base` with the fields the FrameParams sets."""
    return dataclasses.replace(base, **{ORACLE_FIELD[k]: v for k, v in dataclasses.asdict(fp).items() if v is not None})


def params_of(s, fields=("intensity", "thicknessModifier", "projection00")):
    """The FrameParams that sets `fields` to what Settings `s` holds (the inverse of frame_settings)."""
    from miniengineao_amd import FrameParams
    return FrameParams(**{k: getattr(s, ORACLE_FIELD[k]) for k in fields})


def ao_dtype(ao_format):
    return np.uint8 if ao_format == 0 else np.uint16          # L.AO_R8, else f16 bits


def ptr_array(ptrs):
    import ctypes as C
    return (C.c_void_p * len(ptrs))(*ptrs)


def colour(w, h, seed):
    """RGBA16F bits: finite halfs of every sign and size."""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 0x7C00, (h, w, 4)) | (rng.integers(0, 2, (h, w, 4)) << 15)).astype(np.uint16)


def encode_depth(d, fmt):
    """Raw f32 depth in a depth-buffer storage format (L.DEPTH_F32 / _UNORM16 / _UNORM24 / _F16), clipped to [0, 1] for the UNORM
    ones.  Bit-equal to oracle.encode_depth for F32, UNORM16 and F16 on the suites' frames; its UNORM24 codes are the oracle's
    without the 0xA5 stencil byte that the oracle plants above them."""
    if fmt == 0:
        return d.astype(np.float32)
    if fmt == 1:
        return np.round(np.clip(d, 0, 1) * 65535).astype(np.uint16)
    if fmt == 2:
        return np.round(np.clip(d, 0, 1).astype(np.float64) * 16777215).astype(np.uint32)
    return d.astype(np.float16).view(np.uint16)


def downsample_ms(ao, call):
    """The DOWNSAMPLE slot of one call, in a profiling window of its own: 0 = that call launched no downsample pass."""
    ao.set_profiling(True)
    call()
    ms, execs = ao.pass_times_ms()
    assert execs == 1
    return ms[PASS_DOWNSAMPLE]


_WANT, _AO = {}, {}


def want_of(oracle, key, depth, s, result_only=False, **kw):
    """oracle.run(depth, s), computed once per (frame key, every field of s, result_only) and never modified: the oracle is the
    slow part of the GPU suites.  `key` names the frame's contents; their checksum keeps suites with like keys apart."""
    k = (key, checksum(depth), dataclasses.astuple(s), result_only)
    if k not in _WANT:
        _WANT[k] = oracle.run(depth, s, result_only=result_only, **kw)
    return _WANT[k]


def oracle_frame(oracle, w, h, ao_format, seed):
    """(depth, oracle AO) of one synthetic frame; cached."""
    key = (w, h, ao_format, seed)
    if key not in _AO:
        depth = synth.make("S2", w, h, seed=seed)
        _AO[key] = (depth, oracle.run(depth, settings(oracle, w, h, ao_format=ao_format), result_only=True)["result"])
    return _AO[key]


def checksum(arr: np.ndarray) -> int:
    """Order-sensitive 64-bit checksum (FNV-style fold of 8-byte words) used for goldens."""
    b = np.ascontiguousarray(arr).view(np.uint8).ravel()
    pad = (-len(b)) % 8
    if pad:
        b = np.concatenate([b, np.zeros(pad, np.uint8)])
    w = b.view(np.uint64)
    idx = np.arange(1, len(w) + 1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        mixed = (w ^ (idx * np.uint64(0x9E3779B97F4A7C15))) * np.uint64(0x100000001B3)
        return int(np.bitwise_xor.reduce(mixed) ^ np.uint64(len(b)))


# ---- hostile depth inputs (tests/test_hostile_depth.py, tools/fuzz_gpu.py)

def nan_aware_equal(got, want):
    if got.dtype == np.float32:
        g, w = got.view(np.uint32), want.view(np.uint32)
        gn = (g & 0x7fffffff) > 0x7f800000
        wn = (w & 0x7fffffff) > 0x7f800000
    elif got.dtype == np.uint16:      # f16 bit patterns (depth mips, fp16 AO)
        g, w = got, want
        gn = (g & 0x7fff) > 0x7c00
        wn = (w & 0x7fff) > 0x7c00
    else:
        return np.array_equal(got, want), got != want
    bad = ~((g == w) | (gn & wn))
    return not bad.any(), bad


def hostile_values(cam=synth.DEFAULT_CAMERA):
    """{kind: raw depth value} of the hostile texels (hostile_frame; tests/white_tiles.py examines every kind on the oracle)."""
    fpn = np.float32(cam.far) / np.float32(cam.near)
    zp0 = (fpn - np.float32(1)) if cam.reversed_z else (np.float32(1) - fpn)
    zp1 = np.float32(1) if cam.reversed_z else fpn
    zero_den = np.float32(-zp1 / zp0)          # ZBufferParams.x * d + ZBufferParams.y == 0 (or nearly)
    return {
        "nan": np.float32(np.nan), "pinf": np.float32(np.inf), "ninf": np.float32(-np.inf),
        "neg": np.float32(-0.25), "big": np.float32(7.5), "huge": np.float32(3e38), "nhuge": np.float32(-3e38),
        "denorm": np.float32(1e-41), "negzero": np.float32(-0.0), "zero_den": zero_den,
        "tiny_den": np.nextafter(zero_den, np.float32(0), dtype=np.float32), "one": np.float32(1.0),
        "zero": np.float32(0.0),
    }


def hostile_frame(w, h, seed, cam=synth.DEFAULT_CAMERA, density=0.01, kinds=None):
    """S2 frame with hostile texels sprinkled in (isolated ones and small blocks)."""
    rng = np.random.default_rng(seed)
    d = synth.make("S2", w, h, seed=seed).copy()
    values = hostile_values(cam)
    names = list(values) if kinds is None else list(kinds)
    n = max(1, int(w * h * density))
    ys, xs = rng.integers(0, h, n), rng.integers(0, w, n)
    for i in range(n):
        v = values[names[i % len(names)]]
        if i % 7 == 0:
            d[ys[i]:ys[i] + 3, xs[i]:xs[i] + 5] = v
        else:
            d[ys[i], xs[i]] = v
    return d


def hostile_level_texels(w, h, seed):
    """S2 with hostile raw texels only where (y, x) are both even: the texels the levels are made of."""
    clean = synth.make("S2", w, h, seed=seed)
    d = hostile_frame(w, h, seed, density=0.02)
    yy, xx = np.mgrid[0:h, 0:w]
    return np.where(((yy & 1) == 0) & ((xx & 1) == 0), d, clean).astype(np.float32)


def flat_sky_frame(w, h, seed, cam=synth.DEFAULT_CAMERA):
    """S2 with flat regions made of whole 2 x 2-aligned blocks (every level's hi == lo there: |delta| = 0) and sky texels."""
    d = synth.make("S2", w, h, seed=seed).copy()
    d[32:96, 64:192] = d[32, 64]
    d[130:162, 300:364] = d[130, 300]
    d[64:66, 400:402] = d[64, 400]
    sky = np.float32(0.0 if cam.reversed_z else 1.0)
    d[180:232, 100:164] = sky
    d[7:9, 9:13] = sky
    return d


# ---- the parameter domain (tests/test_abi.py, tests/test_param_domain_gpu.py, tools/fuzz_gpu.py)

# values far outside the inspector ranges of AmbientOcclusion.cs (still valid: any finite value is accepted): overflow and
# underflow of 10^x, zero and negative thickness / intensity
FAR_OUTSIDE = {"upsample_tolerance": (-20.0, -40.0, -46.0, 20.0, 39.0), "noise_filter_tolerance": (-46.0, 20.0, 39.0),
               "blur_tolerance": (-46.0, 3.0, 39.0), "thickness_modifier": (-1.0, 1e-30, 1e30), "intensity": (-1.0, 3.0, 1e30)}


def f32(x):
    return float(np.float32(x))


def random_params(rng, w, h, n):
    """n FrameParams with all ten fields drawn from their valid ranges, plus the extremes."""
    from miniengineao_amd import FrameParams
    out = []
    for f in range(n):
        near = f32(10 ** rng.uniform(-2, 0))
        far = f32(near * 10 ** rng.uniform(1, 4))
        fov = rng.uniform(20, 100)
        out.append(FrameParams(
            nearClipPlane=near, farClipPlane=far,
            projection00=synth.Camera(near, far, fov).proj00(w, h),
            usesReversedZBuffer=bool(rng.integers(0, 2)), singlePassStereoEnabled=bool(rng.integers(0, 2)),
            intensity=f32(rng.uniform(0, 4)), thicknessModifier=f32(rng.uniform(1, 10)),
            noiseFilterTolerance=f32(rng.uniform(-8, 0)), blurTolerance=f32(rng.uniform(-8, -1)),
            upsampleTolerance=f32(rng.uniform(-12, -1))))
    ext = [dict(nearClipPlane=0.01, farClipPlane=1e5, usesReversedZBuffer=True, upsampleTolerance=-1.0, noiseFilterTolerance=-8.0),
           dict(nearClipPlane=0.01, farClipPlane=1e5, usesReversedZBuffer=False, upsampleTolerance=-12.0, noiseFilterTolerance=0.0),
           dict(usesReversedZBuffer=False, upsampleTolerance=-12.0, noiseFilterTolerance=-8.0),
           dict(usesReversedZBuffer=True, upsampleTolerance=-1.0, noiseFilterTolerance=0.0)]
    for i, e in enumerate(ext[:n]):
        out[i] = dataclasses.replace(out[i], **e)
    return out


def upsample_constants(lib, w=516, h=260, level=1, **fields):
    """meao_upsample_constants_for with the default parameters and `fields` (meao_params names)."""
    import ctypes as C
    from miniengineao_amd import _lib as L
    p = L.Params()
    lib.meao_default_params(C.byref(p))
    for k, v in fields.items():
        setattr(p, k, v)
    u = L.UpsampleConstants()
    assert lib.meao_upsample_constants_for(w, h, C.byref(p), level, C.byref(u)) == 0
    return u


def in_exact_range(lib, **fields):
    """Whether a context with these parameters divides with the exact v_rcp_f32 sequences under RTZ storage: the range
    meao_api.cpp exact_rcp_div_applicable accepts for the upsample constants."""
    u = upsample_constants(lib, **fields)
    return 2.0 ** -44 <= u.upsample_tolerance <= 2.0 ** 20 and 2.0 ** -30 <= u.noise_filter_strength <= 2.0 ** 50


def exact_range_edges(lib):
    """{edge: (last float32 value inside the exact range, first one outside)}, bisected over float32 values on the library's
    own constants: upsampleTolerance below and above, noiseFilterTolerance above (at the default upsampleTolerance)."""
    def edge(field, inside, outside):
        inside, outside = np.float32(inside), np.float32(outside)
        assert in_exact_range(lib, **{field: float(inside)}) and not in_exact_range(lib, **{field: float(outside)})
        while np.nextafter(inside, outside, dtype=np.float32) != outside:
            mid = np.float32((float(inside) + float(outside)) / 2)
            if mid in (inside, outside):
                mid = np.nextafter(inside, outside, dtype=np.float32)
            if in_exact_range(lib, **{field: float(mid)}):
                inside = mid
            else:
                outside = mid
        return float(inside), float(outside)
    return {"upsample_low": ("upsample_tolerance",) + edge("upsample_tolerance", -12.0, -16.0),
            "upsample_high": ("upsample_tolerance",) + edge("upsample_tolerance", 0.0, 8.0),
            "noise_high": ("noise_filter_tolerance",) + edge("noise_filter_tolerance", 0.0, 12.0)}


# ---- which kernels a child process launches (rocprofv3 kernel trace)

def kernel_trace(tmp_path, script, args=()):
    """Runs `script` (Python source) as a child under rocprofv3 --kernel-trace.  Returns a Count: launches of kernel template
    `name` by count["name"]; .names: the trace's kernel names in start order; .short: those of the meao kernels normalised the
    way tests/kernel_inventory.py names the library's instantiations; .stdout / .stderr of the child."""
    import csv
    import glob
    import os
    import shutil
    import subprocess
    import sys

    import pytest
    prof = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if prof is None:
        pytest.skip("rocprofv3 is not installed")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tmp_path.mkdir(parents=True, exist_ok=True)           # a sub-directory of the test's tmp_path: one per trace of a test
    src = tmp_path / "child.py"
    src.write_text(script)
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([prof, "--kernel-trace", "--output-format", "csv", "-d", str(tmp_path / "kt"), "-o", "kt", "--",
                        sys.executable, str(src), *args], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    files = glob.glob(str(tmp_path / "kt" / "**" / "*kernel_trace.csv"), recursive=True)
    assert files, r.stdout[-2000:]
    rows = []
    for f in files:
        with open(f) as fh:
            rows += [(int(row.get("Start_Timestamp") or 0), row["Kernel_Name"]) for row in csv.DictReader(fh)]
    names = [n for _, n in sorted(rows, key=lambda t: t[0])]

    class Count(dict):
        """launches of kernel template `name`, demangled (::name<) or mangled (<len>nameI) in the trace"""
        def __missing__(self, name):
            return sum(1 for k in names if "::%s<" % name in k or "%d%sI" % (len(name), name) in k)

        def __repr__(self):
            return repr(sorted({k[:90] for k in names}))
    from tests import kernel_inventory
    count = Count()
    count.names, count.short, count.stdout, count.stderr = names, kernel_inventory.normalise(names), r.stdout, r.stderr
    return count


def run_against_testhooks(script):
    """Run tests/<script> in its own process against the `testhooks` variant library (-DMEAO_TESTING=1: the only build that exports
    meao_test_*).  The library is built on the spot when it is missing -- a GPU run must never skip these checks silently
     -- and its absence after that is a failure, not a skip."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "miniengineao_amd", "lib", "variants", "libmeao_testhooks.so")
    if not os.path.exists(lib):
        from miniengineao_amd import build
        build.build_variants(["testhooks"], strict=True)
    assert os.path.exists(lib), "the testhooks variant library could not be built"
    proc = subprocess.run([sys.executable, os.path.join(root, "tests", script)], cwd=root,
                          env=dict(os.environ, MEAO_LIB_PATH=lib), capture_output=True, text=True, timeout=900)
    assert proc.returncode == 0, (proc.stdout[-1500:], proc.stderr[-1500:])
