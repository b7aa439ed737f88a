"""FrameStream on the GPU: every frame a stream yields is compared bit for bit with the CPU oracle run on that frame with that
frame's settings (oracle.run through tests/helpers.want_of, which the dynamic-resolution suite shares: same frames, same keys).

Shapes: 384 x 256 (A: W % 8 == 0, the next step's pass rides inside the last kernel), 200 x 120 (B: its tiles fit under A's),
380 x 250 (C3: W % 8 != 0, the carried pass runs as a launch of its own), inside the reservation 400 x 272; batch 2, so that seven
frames end in a partial step.  The camera of a stream is fixed (one proj00, A's) -- a property change would drop the
announcement -- so the oracle's Settings of another size take that proj00, as in tests/dynamic_resolution.Stream."""
import dataclasses

import numpy as np
import pytest

from miniengineao_amd import FrameParams
from miniengineao_amd import _lib as L
from tests import helpers as H
from tests.dynamic_resolution import A, B, C3, RES, call_frames, want_of

pytestmark = pytest.mark.gpu

SIZES = [A, B, A, C3, B, A]


def stream_for(s, **kw):
    """A FrameStream configured like oracle Settings ``s`` (what H.component does for AmbientOcclusion)."""
    from miniengineao_amd import FrameStream
    fs = FrameStream(s.width, s.height, batch=2, num_levels=s.num_levels, ao_format=s.ao_format, f16_rounding=s.f16_rounding,
                     near_clip=s.near_clip, far_clip=s.far_clip, projection00=s.proj00, reversed_z=s.reversed_z,
                     depth_format=s.depth_format, **kw)
    fs.ao.noiseFilterTolerance, fs.ao.blurTolerance, fs.ao.upsampleTolerance = s.noise_filter_tolerance, s.blur_tolerance, s.upsample_tolerance
    fs.ao.thicknessModifier, fs.ao.intensity = s.thickness_modifier, s.intensity
    return fs


def seven(w, h):
    """[(key, raw f32 frame)] x 7 of one size: the frames of four calls of the dynamic-resolution suite."""
    out = []
    for k in (100, 102, 105, 200):
        out += [((k, f), d) for f, d in enumerate(call_frames(k, w, h))]
    return out[:7]


def settings_at(oracle, w, h, **kw):
    s = H.settings(oracle, w, h, **kw)
    s.proj00 = H.settings(oracle, *A).proj00           # the stream's one camera
    return s


def host_bits(x):
    """A yielded frame as the oracle's array type: uint8, or the f16 bits as uint16."""
    if isinstance(x, np.ndarray):
        return x
    a = x.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.float16 else a


def check(oracle, got, keyed, s_of, kind):
    assert len(got) == len(keyed)
    for i, (g, (key, raw)) in enumerate(zip(got, keyed)):
        s = s_of(i, raw)
        depth = oracle.encode_depth(raw, s.depth_format) if s.depth_format != L.DEPTH_F32 else raw
        want = want_of(oracle, depth, s, key)["result"]
        assert isinstance(g, kind), (i, type(g))
        g = host_bits(g)
        assert g.dtype == want.dtype and g.shape == want.shape, (i, g.dtype, g.shape)
        assert np.array_equal(g, want), (i, key, H.diff_report("result", g, want))


HOST_VARIANTS = {"r8": (A, dict()), "f16": (A, dict(ao_format=L.AO_F16)), "unorm16_380x250": (C3, dict(depth_format=L.DEPTH_UNORM16))}


@pytest.mark.parametrize("variant", sorted(HOST_VARIANTS))
def test_host_frames_are_exact(oracle, variant):
    (w, h), skw = HOST_VARIANTS[variant]
    s = H.settings(oracle, w, h, **skw)
    keyed = seven(w, h)
    frames = [oracle.encode_depth(d, s.depth_format) if "depth_format" in skw else d for _, d in keyed]
    with stream_for(s) as fs:
        got = list(fs.run(iter(frames)))
        assert fs.stats == dict(steps=4, frames=7, announced=3, sized_announcements=0, resizes=0)
        check(oracle, got, keyed, lambda i, raw: s, np.ndarray)
        assert all(g.flags.owndata and g.flags.writeable for g in got)
        again = list(fs.run(frames[:3]))                # the stream is reusable; the slots are the same ones
        check(oracle, again, keyed[:3], lambda i, raw: s, np.ndarray)
        assert fs.stats["steps"] == 6 and fs.stats["frames"] == 10


@pytest.mark.parametrize("layout", ["packed", "cropped_stride_512"])
def test_device_frames_are_exact(oracle, layout):
    import torch
    s = H.settings(oracle, *A)
    keyed = seven(*A)
    if layout == "packed":
        frames = [torch.from_numpy(d).cuda() for _, d in keyed]
    else:
        wide = torch.full((7, A[1] + 8, 512), float("nan"), dtype=torch.float32, device="cuda")
        frames = [wide[i, 4:4 + A[1], 64:64 + A[0]] for i in range(7)]
        for t, (_, d) in zip(frames, keyed):
            t.copy_(torch.from_numpy(d))
        assert frames[0].stride(0) == 512 and not frames[0].is_contiguous()
    with stream_for(s) as fs:
        got = list(fs.run(frames))
        check(oracle, got, keyed, lambda i, raw: s, torch.Tensor)      # .cpu() on the current stream: no other wait
        assert all(g.dtype == torch.uint8 and g.device == frames[0].device for g in got)
        assert fs.stats == dict(steps=4, frames=7, announced=3, sized_announcements=0, resizes=0)


@pytest.mark.parametrize("location", ["host", "device"])
def test_size_changes_inside_max_size(oracle, location):
    import torch
    keyed = [((100 + k, f), d) for k, (w, h) in enumerate(SIZES) for f, d in enumerate(call_frames(100 + k, w, h))]
    frames = [d if location == "host" else torch.from_numpy(d).cuda() for _, d in keyed]
    with stream_for(settings_at(oracle, *A), max_size=RES) as fs:
        assert fs.ao.capacity == RES
        got = list(fs.run(frames))
        check(oracle, got, keyed, lambda i, raw: settings_at(oracle, raw.shape[1], raw.shape[0]), np.ndarray if location == "host" else torch.Tensor)
        assert fs.stats == dict(steps=6, frames=12, announced=5, sized_announcements=5, resizes=5)
        assert (fs.ao.width, fs.ao.height) == A


def test_per_frame_cameras(oracle):
    base = H.settings(oracle, *A)
    cams = [FrameParams(nearClipPlane=0.1, farClipPlane=500.0, projection00=base.proj00 * 1.25),
            FrameParams(nearClipPlane=0.5, farClipPlane=2000.0, projection00=base.proj00 * 0.8),
            FrameParams(nearClipPlane=0.3, farClipPlane=100.0, projection00=base.proj00 * 1.5)]
    keyed = seven(*A)[:6]
    fps = [cams[i % 3] for i in range(6)]
    with stream_for(base) as fs:
        got = list(fs.run((d, fp) for (_, d), fp in zip(keyed, fps)))
        check(oracle, got, keyed, lambda i, raw: H.frame_settings(base, fps[i]), np.ndarray)
        # a step with parameters and one without do not share a call
        mixed = [(keyed[0][1], fps[0]), (keyed[1][1], fps[1]), keyed[2][1], (keyed[3][1], None), (keyed[4][1], fps[2])]
        got = list(fs.run(mixed))
        check(oracle, got, keyed[:5], lambda i, raw: H.frame_settings(base, fps[i]) if i in (0, 1) else (H.frame_settings(base, fps[2]) if i == 4 else base), np.ndarray)


def test_host_and_device_frames_alternate(oracle):
    import torch
    s = H.settings(oracle, *A)
    keyed = (seven(*A) + seven(*A))[:12]
    frames = [d if (i // 3) % 2 == 0 else torch.from_numpy(d).cuda() for i, (_, d) in enumerate(keyed)]
    with stream_for(s) as fs:
        got = list(fs.run(frames))
        assert [type(g) for g in got] == [np.ndarray if (i // 3) % 2 == 0 else torch.Tensor for i in range(12)]
        check(oracle, got, keyed, lambda i, raw: s, (np.ndarray, torch.Tensor))
        assert fs.stats["steps"] == 8 and fs.stats["announced"] == 7       # blocks of three at batch 2: steps of 2 + 1 frames


TRACE_CHILD = r"""
import torch
from miniengineao_amd import FrameStream
A, B, C3 = (384, 256), (200, 120), (380, 250)
frame = lambda s: torch.full((s[1], s[0]), 0.5, dtype=torch.float32, device="cuda")
with FrameStream(*A, batch=2) as fs:
    out = list(fs.run(frame(A) for _ in range(8)))
    torch.cuda.synchronize()
    assert fs.stats["steps"] == 4 and len(out) == 8
with FrameStream(*A, batch=2, max_size=(400, 272)) as fs:
    out = list(fs.run(frame(s) for s in (A, B, A, C3, B, A) for _ in range(2)))
    torch.cuda.synchronize()
    assert fs.stats["steps"] == 6 and fs.stats["resizes"] == 5 and len(out) == 12
"""


def test_the_stream_stays_pipelined(tmp_path):
    """Launches by kernel name.  Four full uniform steps: the first runs its own downsample pass, three carry the next step's in
    their last kernel, the last carries nothing.  Then the size-change stream: carried or as a launch of its own, every step's
    pass runs exactly once -- none re-run, none missing."""
    from tests import kernel_inventory
    count = H.kernel_trace(tmp_path, TRACE_CHILD)
    bases = [kernel_inventory.split(n)[0] for n in count.short]
    finals = [i for i, b in enumerate(bases) if b.startswith("upsample_final")]
    assert len(finals) == 4 + 6, count.short                  # one last kernel per call
    first, second = bases[:finals[3] + 1], bases[finals[3] + 1:]

    def tally(names):
        carried = sum(b.startswith("upsample_final_with_next_downsample") for b in names)
        return dict(downsample=sum(b.startswith("downsample") for b in names), carried=carried,
                    other_final=sum(b.startswith("upsample_final") for b in names) - carried)
    assert tally(first) == dict(downsample=1, carried=3, other_final=1), first
    t = tally(second)
    assert t["downsample"] + t["carried"] == 6 and t["carried"] + t["other_final"] == 6, (t, second)
    assert t["carried"] >= 1                                   # A -> B rides inside A's last kernel


def test_errors_name_the_frame_and_leave_the_device_usable(oracle):
    import torch
    s = settings_at(oracle, *A)
    keyed = seven(*A)
    good = [d for _, d in keyed]

    def works_afterwards():
        with stream_for(s) as fs2:
            check(oracle, list(fs2.run(good[:3])), keyed[:3], lambda i, raw: s, np.ndarray)

    # a frame larger than max_size: the five frames in front of it are yielded, exact, then the error
    fs = stream_for(s, max_size=RES)
    got = []
    with pytest.raises(ValueError, match=r"frame 5: 401 x 272 .*max_size"):
        for g in fs.run(good[:5] + [np.zeros((272, 401), np.float32)] + good[5:]):
            got.append(g)
    check(oracle, got, keyed[:5], lambda i, raw: s, np.ndarray)
    fs.close()
    works_afterwards()
    # without max_size a changed size is refused, and the message says what to do
    fs = stream_for(s)
    with pytest.raises(ValueError, match=r"frame 1: 200 x 120 .*max_size="):
        list(fs.run([good[0], np.zeros((120, 200), np.float32)]))
    fs.close()
    # a wrong dtype, a CPU tensor, a frame of the wrong rank, rows that are not contiguous
    for bad, pattern in ((good[1].astype(np.float64), r"frame 2: dtype float64"),
                         (torch.from_numpy(good[1]), r"frame 2: a tensor on cpu"),
                         (good[1][None], r"frame 2: expected an \(H, W\) array"),
                         (np.asfortranarray(good[1]), r"frame 2: texels of a row are not contiguous"),
                         (torch.from_numpy(good[1]).cuda().double(), r"frame 2: dtype torch.float64")):
        fs = stream_for(s)
        got = []
        with pytest.raises(ValueError, match=pattern):
            for g in fs.run([good[0], good[1], bad, good[2]]):
                got.append(g)
        check(oracle, got, keyed[:2], lambda i, raw: s, np.ndarray)
        fs.close()
    works_afterwards()
    # a property of the context while a run is active
    fs = stream_for(s)
    run = fs.run(good)
    first = next(run)
    with pytest.raises(ValueError, match=r"intensity cannot change while FrameStream.run is active \(frame 1 "):
        fs.ao.intensity = 2.0
    assert fs.ao.intensity == s.intensity
    check(oracle, [first] + list(run), keyed, lambda i, raw: s, np.ndarray)     # the run goes on untouched
    fs.ao.intensity = 2.0                                                       # between runs it is an ordinary property
    louder = dataclasses.replace(s, intensity=2.0)
    check(oracle, list(fs.run(good[:2])), keyed[:2], lambda i, raw: louder, np.ndarray)
    fs.close()
    works_afterwards()


def test_clean_end_and_abandoned_run(oracle):
    import torch
    s = H.settings(oracle, *A)
    keyed = seven(*A)
    with stream_for(s) as fs:
        got = list(fs.run(torch.from_numpy(d).cuda() for _, d in keyed))
        check(oracle, got, keyed, lambda i, raw: s, torch.Tensor)
        assert not fs.ao.composite_pending
        # no stale announcement is consumed or carried: a plain call runs its own pass and is exact
        ms = H.downsample_ms(fs.ao, lambda: check(oracle, [fs.ao.render(keyed[3][1])], keyed[3:4], lambda i, raw: s, np.ndarray))
        assert ms > 0
        fs.ao.set_profiling(False)
        # a run abandoned with steps in flight leaves nothing announced either
        run = fs.run(d for _, d in keyed)
        check(oracle, [next(run)], keyed[:1], lambda i, raw: s, np.ndarray)
        run.close()
        ms = H.downsample_ms(fs.ao, lambda: check(oracle, [fs.ao.render(keyed[4][1])], keyed[4:5], lambda i, raw: s, np.ndarray))
        assert ms > 0
        fs.ao.set_profiling(False)
        check(oracle, list(fs.run(d for _, d in keyed)), keyed, lambda i, raw: s, np.ndarray)
