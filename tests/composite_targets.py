"""The three surfaces of a composite -- AO (an input), colour, GBuffer0 -- as tests/gpu_kit.py Surfaces, for the composite suites
(tests/test_composite_pitched_gpu.py, tests/test_composite_formats_gpu.py, tests/test_composite_batch_gpu.py)."""
import numpy as np

from tests import color_formats as CF
from tests import helpers as H
from tests.gpu_kit import Surface

GUARD = 256


def typed(raw, fmt):
    """(h, w, texel bytes) uint8 -> the view of a colour surface that tests/color_formats.py and oracle.composite take."""
    raw = np.ascontiguousarray(raw)
    if fmt == CF.RGBA32F:
        return raw.view(np.float32)
    if fmt == CF.RGBA8:
        return raw
    if fmt == CF.R11G11B10F:
        return raw.view(np.uint32)[..., 0]
    return raw.view(np.uint16)


def raw_of(c, fmt, h, w):
    return np.ascontiguousarray(c).view(np.uint8).reshape(h, w, CF.TEXEL_BYTES[fmt])


class Targets:
    """n frames of AO (an input), colour in `fmt` and RGBA8 GBuffer0 viewports inside larger surfaces filled with 0xA5: one Surface
    each (.ao, .color, .g), the frames adjacent, GUARD bytes around.  layout = ((x0, pitch) of the AO, the colour and the GBuffer0
    surface in texels, y0, rows, the bytes the colour allocation is shifted by): the suites' kind tables.  ao_frames as the oracle
    gives them; color_frames as (h, w, texel bytes) uint8; a suite that holds them otherwise converts with typed() / raw_of()."""

    def __init__(self, w, h, fmt, ao_format, kind, layout, ao_frames, color_frames, g_frames, device="cuda"):
        self.w, self.h, self.fmt, self.ao_format, self.kind, self.n = w, h, fmt, ao_format, kind, len(ao_frames)
        self.want_ao, self.color0, self.gbuf0 = ao_frames, color_frames, g_frames
        (a, c, g), y0, rows, shift = layout
        ao_dt = np.uint8 if ao_format == CF.AO_R8 else np.uint16

        def surface(dtype, tail, origin, frames, shift=0):
            return Surface(w, h, dtype, tail, n=self.n, pitch=origin[1], x0=origin[0], y0=y0, rows=rows, guard=GUARD, shift=shift,
                           content=frames, device=device)
        self.ao = surface(ao_dt, (), a, [np.ascontiguousarray(f).view(ao_dt) for f in ao_frames])
        self.color = surface(np.uint8, (CF.TEXEL_BYTES[fmt],), c, color_frames, shift)
        self.g = surface(np.uint8, (4,), g, g_frames)

    # what a call takes: 0 for packed rows
    ao_pitch = property(lambda self: self.ao.pitch_bytes)
    color_pitch = property(lambda self: self.color.pitch_bytes)
    g_pitch = property(lambda self: self.g.pitch_bytes)

    def ao_ptrs(self, base=None):
        return self.ao.ptrs(base)

    def color_ptrs(self, base=None):
        return self.color.ptrs(base)

    def g_ptrs(self, base=None):
        return self.g.ptrs(base)

    def expected(self, mode, f, with_g=True):
        """(colour as (h, w, texel bytes) uint8, GBuffer0) of frame f composited in `mode`: the model tests/color_formats.py applied
        to the oracle's AO; RGBA16F, which the model does not cover: oracle.composite."""
        g0 = self.gbuf0[f] if mode == 1 and with_g else None
        if self.fmt == CF.RGBA16F:
            from oracle import oracle as O
            c, g = typed(self.color0[f], self.fmt).copy(), None if g0 is None else g0.copy()
            O.composite(np.ascontiguousarray(self.want_ao[f]), c, mode, self.ao_format, g)
        else:
            c, g = CF.composite(self.want_ao[f], self.ao_format, typed(self.color0[f], self.fmt), self.fmt, mode, g0)
        return raw_of(c, self.fmt, self.h, self.w), (g if g is not None else self.gbuf0[f])

    def same_color(self, got, want, nan_limit, what):
        """An RGBA32F channel whose expected value is NaN is compared for NaN-ness only (host and device multiply may differ in
        payload); every other bit of every format must be equal."""
        if self.fmt == CF.RGBA32F:
            gw, ww = got.view(np.uint32).copy(), np.ascontiguousarray(want).view(np.uint32).copy()
            nan = np.isnan(ww.view(np.float32))
            assert nan_limit is None or int(nan.sum()) <= nan_limit, "at most the probe texel's four channels fall under the NaN rule"
            assert np.array_equal(np.isnan(gw.view(np.float32)), nan), (what, "NaN-ness")
            gw[nan], ww[nan] = 0, 0
            got, want = gw, ww
        assert np.array_equal(got, want), (what, H.diff_report("color", got, want))

    def check(self, mode, frames=None, color=None, g=None, ao=None, nan_limit=4):
        """Frames `frames` (default: all) composited in `mode`, the others as uploaded; color, g, ao: the bytes of the whole
        allocations, default the device's.  nan_limit: how many channel values of a frame may fall under the NaN rule (None: the
        frame is made of such values on purpose)."""
        if self.color.dev is not None:
            import torch
            torch.cuda.synchronize()
        color = self.color.download() if color is None else color
        g = self.g.download() if g is None else g
        ao = self.ao.download() if ao is None else ao
        assert np.array_equal(ao, self.ao.host), "the AO surface is an input"
        frames = range(self.n) if frames is None else frames
        for f in range(self.n):
            want_c, want_g = self.expected(mode, f) if f in frames else (self.color0[f], self.gbuf0[f])
            what = (self.kind, self.fmt, mode, f)
            self.same_color(self.color.view(f, color), want_c, nan_limit, what)
            assert np.array_equal(self.g.view(f, g), want_g), (what, H.diff_report("gbuffer0", self.g.view(f, g), want_g))
        assert self.color.intact(color), "colour bytes outside the viewports changed"
        assert self.g.intact(g), "GBuffer0 bytes outside the viewports changed"


class Renders:
    """Depth frames on the device and somewhere for the AO of the calls that carry (or push out) a composite batch.  frames:
    [(depth, the oracle's AO)]; the calls go to the current stream."""

    def __init__(self, frames, ao_format):
        import torch
        self.torch, self.n, self.want = torch, len(frames), [a for _, a in frames]
        self.depth = [torch.from_numpy(d).cuda() for d, _ in frames]
        dt = torch.uint8 if ao_format == CF.AO_R8 else torch.int16
        self.out = [torch.zeros(a.shape, dtype=dt, device="cuda") for _, a in frames]

    def execute(self, ao, n=None, params=None):
        n = self.n if n is None else n
        ao.execute_device([t.data_ptr() for t in self.depth[:n]], [t.data_ptr() for t in self.out[:n]],
                          self.torch.cuda.current_stream().cuda_stream, params=params)

    def check(self, n=None):
        self.torch.cuda.synchronize()
        for f in range(self.n if n is None else n):
            got = self.out[f].cpu().numpy().view(self.want[f].dtype)
            assert np.array_equal(got, self.want[f]), (f, H.diff_report("result", got, self.want[f]))


# ---- the targets of the colour-format suites (tests/test_composite_formats_gpu.py, tests/test_composite_batch_gpu.py)

Y0 = 2


def up4(x):
    return (x + 3) // 4 * 4


def format_layout(kind, w, h):
    """"packed"; "vector" (colour base and pitch multiples of 16 bytes, AO base and pitch multiples of four texels); "scalar" (an odd
    pitch in texels for colour and AO); "oddbase" (vector pitches, the colour base 4 bytes off a 16-byte boundary and the AO base
    one texel off)."""
    table = {"vector": ((4, up4(w + 8)), (4, up4(w + 8)), (1, w + 3)), "scalar": ((1, (w + 4) | 1), (1, (w + 4) | 1), (3, w + 5)),
             "oddbase": ((1, up4(w + 8)), (4, up4(w + 8)), (2, w + 2)), "packed": ((0, w), (0, w), (0, w))}
    return table[kind], (0 if kind == "packed" else Y0), (h if kind == "packed" else h + Y0 + 1), (4 if kind == "oddbase" else 0)


def random_color(rng, fmt, h, w):
    """Random texels of `fmt` as (h, w, texel bytes) uint8, with one probe texel of non-finite and edge values."""
    if fmt == CF.RGBA32F:
        c = (rng.random((h, w, 4)) * 6.0).astype(np.float32)
        c[h // 3, w // 2] = [np.inf, -np.inf, 1e-45, -0.0]
    elif fmt == CF.RGBA8:
        c = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        c[h // 3, w // 2] = [0, 255, 1, 254]
    elif fmt == CF.R11G11B10F:
        c = rng.integers(0, 1 << 32, (h, w), dtype=np.uint64).astype(np.uint32)
        c &= ~np.uint32((0x400 << 0) | (0x400 << 11) | (0x200 << 22))                # exponents below 16: finite values up to 2
        c[h // 3, w // 2] = 0x7C0 | (0x7FF << 11) | (0x001 << 22)                    # inf, NaN, the smallest subnormal
    else:
        c = (rng.random((h, w, 4)) * 6.0).astype(np.float16).view(np.uint16)
    return raw_of(c, fmt, h, w)


class FormatTargets(Targets):
    """Targets in a format_layout, with random colour (unless given) and GBuffer0 texels drawn from `seed`."""

    def __init__(self, w, h, fmt, ao_format, kind, ao_frames, color_frames=None, seed=1, device="cuda"):
        rng = np.random.default_rng(seed)
        n = len(ao_frames)
        color = color_frames if color_frames is not None else [random_color(rng, fmt, h, w) for _ in range(n)]
        g = [rng.integers(0, 256, (h, w, 4), dtype=np.uint8) for _ in range(n)]
        super().__init__(w, h, fmt, ao_format, kind, format_layout(kind, w, h), ao_frames, color, g, device)
