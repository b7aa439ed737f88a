"""Freezes what the reference's own C# host and shader text produce for the small cases of
tests/test_reference_goldens.py, so that those tests run without the reference tree:

  * ref_host_commands.json -- the dispatches (kernel, groups, texture bindings, constant blocks),
    render-texture allocations and result size recorded by the INTERPRETED AmbientOcclusion.cs
    (make_reference_goldens.record_reference_commands) for the host-constant and variant-constant
    cases, the Render.main constant blocks of the non-tiled-source branch, and the kernel sequence of
    the tiny live frame;
  * ref_tiny_18x11.npz     -- all buffers of that tiny frame through the interpreted shaders;
  * ref_mutated_26x15.npz  -- the buffers of a 26x15 frame through copies of the shader text with one
    token changed (MUTATIONS): what shows that the interpreters execute the text.

Constants are float32 values stored as JSON numbers (exact round trip); a texture binding that is not
a named render texture of the component (the camera's depth, the result target) is stored as its type.

    python tests/golden/make_reference_host_goldens.py       # needs the reference tree (make_reference_goldens.SHADERS)
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from miniengineao_amd import synth  # noqa: E402
from tests import helpers as H  # noqa: E402

COMMANDS = os.path.join(HERE, "ref_host_commands.json")
TINY = os.path.join(HERE, "ref_tiny_18x11.npz")
MUTATED = os.path.join(HERE, "ref_mutated_26x15.npz")
HOST_SEEDS = range(6)
VARIANT_SEEDS = range(4)

# (shader, find, replace, buffers that must change)
MUTATIONS = [
    # one sample offset of the checker set: render and everything behind it changes
    ("Render", "TestSamples(thisIdx, 2, 4, invThisDepth, gInvThicknessTable[2].z);\n#endif",
     "TestSamples(thisIdx, 1, 4, invThisDepth, gInvThicknessTable[2].z);\n#endif", ("occlusion1", "combined1", "result")),
    # the blur's centre weight: only the upsample outputs change
    ("Upsample", "/ 2.0 + b + c + d) / 4.0;", "/ 2.0 + b + c + d) / 4.5;", ("combined3", "combined1", "result")),
]


def tiny_case(O):
    w, h = 18, 11
    cam = synth.Camera(reversed_z=False)
    from tests.golden import make_reference_goldens as R
    depth = R.make_depth("S2", w, h, 5, cam, True)
    return depth, H.settings(O, w, h, cam=cam, intensity=0.8, thickness_modifier=3.0)


def mutated_case(O):
    w, h = 26, 15
    cam = synth.DEFAULT_CAMERA
    from tests.golden import make_reference_goldens as R
    depth = R.make_depth("S2", w, h, 9, cam, False)
    return depth, H.settings(O, w, h, cam=cam)


def host_case(O, seed):
    rng = np.random.default_rng(seed)
    w, h = int(rng.integers(17, 4000)), int(rng.integers(9, 2200))
    cam = synth.Camera(near=float(rng.uniform(0.01, 1)), far=float(rng.uniform(5, 2000)),
                       fov_y_deg=float(rng.uniform(10, 100)), reversed_z=bool(seed & 1))
    return H.settings(O, w, h, cam=cam, noise_filter_tolerance=float(rng.uniform(-8, 0)),
                      blur_tolerance=float(rng.uniform(-8, -1)), upsample_tolerance=float(rng.uniform(-12, -1)),
                      thickness_modifier=float(rng.uniform(1, 10)), intensity=float(rng.uniform(0, 2)))


def variant_case(O, seed):
    rng = np.random.default_rng(100 + seed)
    w, h = 2 * int(rng.integers(9, 2000)), int(rng.integers(9, 2200))
    stereo = bool(seed & 1)
    cam = synth.Camera(near=float(rng.uniform(0.01, 1)), far=float(rng.uniform(5, 2000)),
                       fov_y_deg=float(rng.uniform(10, 100)), reversed_z=bool(seed & 2))
    return H.settings(O, w, h, cam=cam, thickness_modifier=float(rng.uniform(1, 10)),
                      intensity=float(rng.uniform(0, 2)), single_pass_stereo=stereo, hq_levels=4), cam


def _settings_key(s):
    return [s.width, s.height, float(s.proj00), float(s.near_clip), float(s.far_clip), bool(s.reversed_z),
            float(s.intensity), float(s.thickness_modifier)]


def _dispatch(d):
    tex = {k: v if isinstance(v, str) else f"<{type(v).__name__}>" for k, v in d["tex"].items()}
    return {"shader": d["shader"], "kernel": d["kernel"], "groups": list(d["groups"]), "tex": tex,
            "const": {k: [float(x) for x in v] for k, v in d["const"].items()}}


def load_commands(kind, seed, O, s):
    """The recorded commands of case (kind, seed) as (cmd, result_rt, hq) with the attributes the tests read;
    asserts that the case's settings are still the ones the fixture was recorded with."""
    from types import SimpleNamespace
    with open(COMMANDS) as f:
        rec = json.load(f)[kind][str(seed)]
    assert rec["settings"] == _settings_key(s), "the case's settings changed: regenerate the fixture"
    cmd = SimpleNamespace(dispatches=[dict(d, groups=tuple(d["groups"])) for d in rec["dispatches"]],
                          allocs={k: tuple(v) for k, v in rec["allocs"].items()})
    rt = SimpleNamespace(width=rec["result_rt"][0], height=rec["result_rt"][1])
    hq = {int(k): {"const": v} for k, v in rec.get("hq", {}).items()}
    return cmd, rt, hq


def main():
    from oracle import oracle as O
    from tests.golden import make_reference_goldens as R
    O.build()
    out = {"host": {}, "variant": {}}
    for seed in HOST_SEEDS:
        s = host_case(O, seed)
        _, cmd, rt = R.record_reference_commands(s)
        out["host"][str(seed)] = {"settings": _settings_key(s), "dispatches": [_dispatch(d) for d in cmd.dispatches],
                                  "allocs": {k: list(v) for k, v in cmd.allocs.items()}, "result_rt": [rt.width, rt.height]}
    for seed in VARIANT_SEEDS:
        s, _ = variant_case(O, seed)
        _, cmd, rt, it, comp = R.record_reference_commands(s, want_interp=True)
        out["variant"][str(seed)] = {"settings": _settings_key(s), "dispatches": [_dispatch(d) for d in cmd.dispatches],
                                     "allocs": {k: list(v) for k, v in cmd.allocs.items()}, "result_rt": [rt.width, rt.height],
                                     "hq": {str(level): _dispatch(R.hq_render_commands(s, it, comp, level))["const"]
                                            for level in (1, 2, 3, 4)}}
    depth, s = tiny_case(O)
    ref, cmd = R.run_reference_shaders(depth, s, log=lambda *_: None)
    out["tiny_kernels"] = [d["kernel"] for d in cmd.dispatches]
    out["mutations"] = [[shader, find, replace] for shader, find, replace, _ in MUTATIONS]
    np.savez_compressed(TINY, depth=depth, **ref)
    src = R.shader_sources()
    depth, s = mutated_case(O)
    bufs = {"depth": depth}
    real = R.shader_sources
    try:
        for shader, find, replace, _ in MUTATIONS:
            assert src[shader].count(find) >= 1, "the mutation site moved"
            mutated = dict(src, **{shader: src[shader].replace(find, replace)})
            R.shader_sources = lambda mutated=mutated: mutated
            ref, _ = R.run_reference_shaders(depth, s, log=lambda *_: None)
            bufs.update({f"{shader}__{k}": v for k, v in ref.items()})
    finally:
        R.shader_sources = real
    np.savez_compressed(MUTATED, **bufs)
    with open(COMMANDS, "w") as f:
        json.dump(out, f, indent=None, separators=(",", ":"))
        f.write("\n")
    print("wrote", COMMANDS, TINY, MUTATED)


if __name__ == "__main__":
    main()
