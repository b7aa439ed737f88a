"""The guarded device surface of the GPU suites.

A Surface is n frames of rows x pitch texels, adjacent in one allocation, each with a w x h viewport at (x0, y0).  `guard` bytes lie
in front of and behind the frames, and `shift` moves the whole body off its alignment inside 16 bytes of slack.  Every byte that is
not a viewport texel holds the byte sentinel `fill` (0xA5); the row padding and the rows above and below of a depth input may hold
a pad word instead (DEPTH_PAD_WORD: a NaN or the all-ones code of the format).  `host` mirrors every byte of the allocation, and
intact() compares every byte outside the viewports with it: row padding, rows above and below, guards and slack alike.

A suite that wants one allocation per frame (mixed sizes) makes a list of Surfaces with n = 1.  What a suite's layouts are -- its
pitch kinds, origins and shifts -- stays with the suite: test data.  A SparseSurface is the same guarded frame without the host
mirror, for allocations of gigabytes (tests/test_address_limits_gpu.py).  tests/test_gpu_kit.py checks both checkers on the CPU."""
from __future__ import annotations

import numpy as np

SENTINEL = 0xA5
SLACK = 16                   # bytes a shifted body may move inside
# by meao depth format (L.DEPTH_F32, _UNORM16, _UNORM24, _F16): what the padding of a depth surface holds
DEPTH_PAD_WORD = {0: 0x7fc00000, 1: 0xffff, 2: 0xffffffff, 3: 0x7e00}


class Surface:
    def __init__(self, w, h, dtype, tail=(), n=1, pitch=None, x0=0, y0=0, rows=None, guard=0, shift=0, fill=SENTINEL,
                 pad_word=None, content=None, device="cuda"):
        """dtype, tail: a texel is an array of shape `tail` of dtype.  pitch (texels) and rows default to the tightest that hold the
        viewport.  content: the n viewports' texels.  device=None: the host mirror only."""
        self.w, self.h, self.dtype, self.tail, self.n = w, h, np.dtype(dtype), tuple(tail), n
        self.x0, self.y0 = x0, y0
        self.pitch = x0 + w if pitch is None else pitch
        self.rows = y0 + h if rows is None else rows
        assert self.pitch >= x0 + w and self.rows >= y0 + h and 0 <= shift <= SLACK
        self.texel_bytes = self.dtype.itemsize * int(np.prod(self.tail, dtype=np.int64))
        self.row_bytes = self.pitch * self.texel_bytes
        self.body_bytes = n * self.rows * self.row_bytes
        self.offset = shift + guard                                  # of the body in the allocation
        self.host = np.full((SLACK if shift else 0) + 2 * guard + self.body_bytes, fill, np.uint8)
        if pad_word is not None:
            word = np.dtype("u%d" % self.dtype.itemsize)
            self.host[self.offset:self.offset + self.body_bytes] = np.full(self.body_bytes // word.itemsize, pad_word, word).view(np.uint8)
        if content is not None:
            self.put(content)
        self.device, self.dev = device, None
        if device is not None:
            self.upload()

    def frames(self, raw=None):
        """The body of `raw` (default: the host mirror) as an (n, rows, pitch) + tail array of texels; a view, writable."""
        raw = self.host if raw is None else raw
        return raw[self.offset:self.offset + self.body_bytes].view(self.dtype).reshape((self.n, self.rows, self.pitch) + self.tail)

    def view(self, f=0, raw=None):
        return self.frames(raw)[f, self.y0:self.y0 + self.h, self.x0:self.x0 + self.w]

    def put(self, content):
        for f, a in enumerate(content):
            self.view(f)[...] = np.asarray(a).reshape((self.h, self.w) + self.tail)

    def upload(self):
        import torch
        self.dev = torch.from_numpy(self.host.copy()).to(self.device)

    def download(self):
        return self.dev.cpu().numpy()

    def ptr_of(self, f=0, base=None):
        """The address of frame f's viewport; base: where a host copy of the allocation lies (default: the device tensor)."""
        base = self.dev.data_ptr() if base is None else base
        return base + self.offset + (f * self.rows + self.y0) * self.row_bytes + self.x0 * self.texel_bytes

    def ptrs(self, base=None):
        return [self.ptr_of(f, base) for f in range(self.n)]

    ptr = property(ptr_of)

    @property
    def packed(self):
        return self.pitch == self.w

    @property
    def pitch_bytes(self):
        """What a call takes as this surface's pitch: 0 for packed rows (row_bytes is the real figure either way)."""
        return 0 if self.packed else self.row_bytes

    def texels(self, f=0, raw=None):
        return self.view(f, self.download() if raw is None else raw).copy()

    def intact(self, raw=None):
        """Whether every byte of `raw` (default: the device's) that is no viewport texel is what the mirror holds."""
        rest = np.array(self.download() if raw is None else raw, copy=True)
        if rest.shape != self.host.shape or rest.dtype != np.uint8:
            return False
        for f in range(self.n):
            self.view(f, rest)[...] = self.view(f)
        return np.array_equal(rest, self.host)

    def read(self, f=0, raw=None):
        """(frame f's viewport texels, intact()) from one download."""
        raw = self.download() if raw is None else raw
        return self.texels(f, raw), self.intact(raw)


CHUNK = 256 << 20            # bytes of a SparseSurface that one step of intact() examines


class SparseSurface:
    """Surface's device-resident sibling for one frame whose rows lie so far apart that the allocation is gigabytes and the
    viewport a few KB: no host mirror.  The allocation is guard + (rows - 1) * row_bytes + (x0 + w) * texel_bytes + guard bytes --
    it ends behind the last row's last viewport texel -- filled with the byte `fill` on the device; the viewport rows are written
    and read through a strided device view, and intact() compares every other byte with `fill` on the device, CHUNK bytes at a
    time (its temporaries are one byte per byte examined), so nothing of the surface's size crosses to the host."""

    def __init__(self, w, h, dtype, tail=(), pitch=None, x0=0, y0=0, rows=None, guard=0, fill=SENTINEL, content=None, device="cuda"):
        import torch
        self.w, self.h, self.dtype, self.tail, self.n = w, h, np.dtype(dtype), tuple(tail), 1
        self.x0, self.y0, self.fill = x0, y0, fill
        self.pitch = x0 + w if pitch is None else pitch
        self.rows = y0 + h if rows is None else rows
        assert self.pitch >= x0 + w and self.rows >= y0 + h
        self.texel_bytes = self.dtype.itemsize * int(np.prod(self.tail, dtype=np.int64))
        self.row_bytes = self.pitch * self.texel_bytes
        self.view_bytes = w * self.texel_bytes                       # of one viewport row
        self.body_bytes = (self.rows - 1) * self.row_bytes + (x0 + w) * self.texel_bytes
        self.offset = guard                                          # of the body in the allocation
        self.first = guard + y0 * self.row_bytes + x0 * self.texel_bytes      # of the viewport in the allocation
        self.nbytes = 2 * guard + self.body_bytes
        self.device = device
        self.dev = torch.full((self.nbytes,), fill, dtype=torch.uint8, device=device)
        if content is not None:
            self.put(content)
        self._settle()

    def _settle(self):
        """The fill and the copies are work torch queues on its stream; a library call on another stream is not ordered behind
        them, so construction and put() return with that work complete (as Surface's upload does)."""
        if self.dev.is_cuda:
            import torch
            torch.cuda.synchronize(self.dev.device)

    def rows_view(self):
        """The viewport as an (h, w * texel_bytes) byte tensor over the allocation."""
        return self.dev.as_strided((self.h, self.view_bytes), (self.row_bytes, 1), self.first)

    def put(self, content):
        """content: the viewport's texels, or a list holding them (as Surface takes its frames)."""
        import torch
        a = content[0] if isinstance(content, (list, tuple)) else content
        a = np.ascontiguousarray(np.asarray(a).reshape((self.h, self.w) + self.tail)).view(np.uint8)
        self.rows_view().copy_(torch.from_numpy(a.reshape(self.h, self.view_bytes).copy()))
        self._settle()

    @property
    def ptr(self):
        return self.dev.data_ptr() + self.first

    def ptrs(self):
        return [self.ptr]

    @property
    def packed(self):
        return self.pitch == self.w

    @property
    def pitch_bytes(self):
        return 0 if self.packed else self.row_bytes

    def texels(self):
        """The viewport's texels: the only download."""
        raw = self.rows_view().cpu().numpy()
        return np.ascontiguousarray(raw).view(self.dtype).reshape((self.h, self.w) + self.tail)

    def _outside(self):
        """(start, count, length, stride) of the byte runs that hold no viewport texel: what lies in front of the viewport, the
        h - 1 runs between the end of one viewport row and the start of the next, what lies behind its last row."""
        last_end = self.first + (self.h - 1) * self.row_bytes + self.view_bytes
        return [(0, 1, self.first, 0), (self.first + self.view_bytes, self.h - 1, self.row_bytes - self.view_bytes, self.row_bytes),
                (last_end, 1, self.nbytes - last_end, 0)]

    def intact(self):
        """Whether every byte that is no viewport texel still holds `fill`; decided on the device."""
        for start, count, length, stride in self._outside():
            if count == 0 or length == 0:
                continue
            if count == 1:                                   # one run: CHUNK bytes at a time
                for at in range(start, start + length, CHUNK):
                    if not bool((self.dev[at:min(at + CHUNK, start + length)] == self.fill).all()):
                        return False
                continue
            step = max(1, CHUNK // length)                   # runs a stride apart: as many as make CHUNK bytes (a run is shorter than
            for k in range(0, count, step):                  # a row: one alone is examined whole)
                runs = self.dev.as_strided((min(step, count - k), length), (stride, 1), start + k * stride)
                if not bool((runs == self.fill).all()):
                    return False
        return True

    def read(self):
        """(the viewport's texels, intact())."""
        return self.texels(), self.intact()
