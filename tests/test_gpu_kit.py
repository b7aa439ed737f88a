"""The checker of the GPU suites checked on the CPU: tests/gpu_kit.py Surface through its host mirror (device=None).  A byte flipped
anywhere outside the viewports must make intact() False; a flipped viewport texel must not, and must show in the texels.  The
same for SparseSurface, whose tensor lives on the CPU here (device="cpu")."""
import numpy as np
import pytest

from tests import gpu_kit

W, H, PITCH, X0, Y0, ROWS, GUARD = 5, 3, 9, 2, 1, 5, 16
TEXELS = [(np.uint8, ()), (np.uint16, ()), (np.uint16, (4,))]


def surface(dtype, tail, n=2, shift=0):
    rng = np.random.default_rng(1)
    content = [rng.integers(0, 200, (H, W) + tail).astype(dtype) for _ in range(n)]
    s = gpu_kit.Surface(W, H, dtype, tail, n=n, pitch=PITCH, x0=X0, y0=Y0, rows=ROWS, guard=GUARD, shift=shift, content=content,
                        device=None)
    return s, content


def regions(s, f):
    """{region: byte offset in the allocation} of one byte in every region outside frame f's viewport."""
    tb, base = s.texel_bytes, s.offset + f * s.rows * s.row_bytes
    at = lambda y, x, b=0: base + y * s.row_bytes + x * tb + b         # noqa: E731
    out = {"front guard, first byte": s.offset - GUARD, "front guard, last byte": s.offset - 1,
           "back guard, first byte": s.offset + s.body_bytes, "back guard, last byte": s.offset + s.body_bytes + GUARD - 1,
           "left of x0": at(Y0, X0 - 1, tb - 1), "left of x0, last row": at(Y0 + H - 1, 0),
           "right of the viewport": at(Y0, X0 + W), "right of the viewport, last row": at(Y0 + H - 1, PITCH - 1, tb - 1),
           "row above": at(Y0 - 1, X0 + 1), "row below": at(Y0 + H, X0 + 1), "row below, last byte": at(ROWS - 1, PITCH - 1, tb - 1)}
    if s.offset > GUARD:
        out["slack in front"] = 0
        out["slack in front, last byte"] = s.offset - GUARD - 1
        out["slack behind"] = s.offset + s.body_bytes + GUARD
        out["slack behind, last byte"] = len(s.host) - 1
    return out


@pytest.mark.parametrize("shift", [0, 4])
@pytest.mark.parametrize("dtype,tail", TEXELS)
def test_a_byte_flipped_outside_the_viewports_is_seen(dtype, tail, shift):
    s, content = surface(dtype, tail, shift=shift)
    assert len(s.host) == (gpu_kit.SLACK if shift else 0) + 2 * GUARD + 2 * ROWS * PITCH * s.texel_bytes
    assert s.read(0, s.host.copy())[1] and s.intact(s.host)
    for f in range(s.n):
        for region, at in regions(s, f).items():
            raw = s.host.copy()
            assert raw[at] == gpu_kit.SENTINEL, (region, at)
            raw[at] ^= 0x01
            texels, intact = s.read(f, raw)
            assert not intact, (f, region)
            assert np.array_equal(texels, content[f]), (f, region)
    assert not s.intact(s.host[:-1]) and not s.intact(np.concatenate([s.host, s.host[:1]]))


@pytest.mark.parametrize("dtype,tail", TEXELS)
def test_a_flipped_viewport_texel_shows_in_the_texels_alone(dtype, tail):
    s, content = surface(dtype, tail, shift=4)
    for f in range(s.n):
        for index in [(0, 0), (H - 1, W - 1), (1, 2)]:
            raw = s.host.copy()
            s.view(f, raw)[index] ^= 1
            assert s.intact(raw) and np.array_equal(s.texels(1 - f, raw), content[1 - f])
            bad = np.argwhere((s.texels(f, raw) != content[f]).reshape(H, W, -1).any(axis=2))
            assert bad.tolist() == [list(index)], (f, index, bad)


def test_addresses_and_pitches():
    s, _ = surface(np.uint16, (4,), shift=4)
    assert s.row_bytes == s.pitch_bytes == PITCH * 8 and not s.packed
    base = s.host.ctypes.data
    for f in range(2):
        assert s.ptr_of(f, base) == s.view(f).ctypes.data == base + 4 + GUARD + ((f * ROWS + Y0) * PITCH + X0) * 8
    assert s.ptrs(base) == [s.ptr_of(0, base), s.ptr_of(1, base)]


def test_packed():
    content = [np.arange(W * H, dtype=np.uint16).reshape(H, W)]
    s = gpu_kit.Surface(W, H, np.uint16, content=content, device=None)
    assert s.packed and s.pitch == W and s.rows == H and s.pitch_bytes == 0 and s.row_bytes == 2 * W
    assert len(s.host) == 2 * W * H and s.ptr_of(0, 1000) == 1000
    texels, intact = s.read(0, s.host)
    assert intact and np.array_equal(texels, content[0])
    g = gpu_kit.Surface(W, H, np.uint16, guard=GUARD, device=None)                # packed rows between guards: all sentinel
    assert g.pitch_bytes == 0 and np.all(g.host == gpu_kit.SENTINEL) and len(g.host) == 2 * W * H + 2 * GUARD
    raw = g.host.copy()
    raw[-1] = 0
    assert g.intact(g.host) and not g.intact(raw)


# ---- SparseSurface: the same questions, asked of a torch tensor on the CPU

SPARSE = [dict(), dict(x0=X0, y0=Y0, rows=ROWS), dict(rows=H + 1)]         # the allocation ends behind the viewport's last texel or later


def sparse(dtype, tail, **kw):
    rng = np.random.default_rng(2)
    content = rng.integers(0, 200, (H, W) + tail).astype(dtype)
    content[0, 0] = content[H - 1, W - 1] = gpu_kit.SENTINEL          # sentinel-valued texels are texels
    kw = dict(dict(pitch=PITCH + kw.get("x0", 0), guard=GUARD), **kw)
    return gpu_kit.SparseSurface(W, H, dtype, tail, content=[content], device="cpu", **kw), content


def sparse_regions(s):
    """{region: byte offset in the allocation} of one byte in every kind of place outside the viewport."""
    tb, vb = s.texel_bytes, s.view_bytes
    row = lambda y: s.first + y * s.row_bytes                          # noqa: E731  (viewport row y's first texel)
    out = {"front guard, first byte": 0, "front guard, last byte": GUARD - 1,
           "back guard, first byte": s.nbytes - GUARD, "back guard, last byte": s.nbytes - 1,
           "row padding, first byte behind row 0": row(0) + vb, "row padding, last byte in front of row 1": row(1) - 1,
           "row padding behind the last row but one": row(H - 2) + vb, "row padding in front of the last row": row(H - 1) - 1,
           "the byte behind the last row's texels": row(H - 1) + vb}
    if s.x0 or s.y0:
        out["in front of the first row's texels"] = row(0) - 1
        out["the body's first byte"] = GUARD
    if s.rows > s.y0 + H:
        out["row below, below the viewport"] = row(H) + tb
        out["the body's last byte"] = s.nbytes - GUARD - 1
    return out


@pytest.mark.parametrize("chunk", [gpu_kit.CHUNK, 64, 7])                  # one step; several runs per step; several steps per run
@pytest.mark.parametrize("kw", SPARSE)
@pytest.mark.parametrize("dtype,tail", TEXELS)
def test_sparse_a_stray_byte_outside_the_viewport_is_seen(monkeypatch, dtype, tail, kw, chunk):
    monkeypatch.setattr(gpu_kit, "CHUNK", chunk)
    s, content = sparse(dtype, tail, **kw)
    assert s.nbytes == 2 * GUARD + (s.rows - 1) * s.row_bytes + (s.x0 + W) * s.texel_bytes == len(s.dev)
    texels, intact = s.read()
    assert intact and texels.dtype == np.dtype(dtype) and np.array_equal(texels, content)
    for region, at in sparse_regions(s).items():
        assert int(s.dev[at]) == gpu_kit.SENTINEL, (region, at)
        s.dev[at] ^= 0x01
        texels, intact = s.read()
        assert not intact, region
        assert np.array_equal(texels, content), region
        s.dev[at] ^= 0x01
        assert s.intact(), region


@pytest.mark.parametrize("kw", SPARSE)
@pytest.mark.parametrize("dtype,tail", TEXELS)
def test_sparse_a_changed_viewport_byte_shows_in_the_texels_alone(dtype, tail, kw):
    s, content = sparse(dtype, tail, **kw)
    for y, x in [(0, 0), (H - 1, W - 1), (1, 2), (0, W - 1), (H - 1, 0)]:
        for b in (0, s.texel_bytes - 1):                                  # a texel's first and last byte
            at = s.first + y * s.row_bytes + x * s.texel_bytes + b
            s.dev[at] ^= 0x01
            texels, intact = s.read()
            bad = np.argwhere((texels != content).reshape(H, W, -1).any(axis=2))
            assert intact and bad.tolist() == [[y, x]], (y, x, b, bad)
            s.dev[at] ^= 0x01
    new = content[::-1, ::-1].copy()
    s.put(new)                                                            # put() again replaces the viewport, nothing else
    texels, intact = s.read()
    assert intact and np.array_equal(texels, new)


def test_sparse_addresses_and_pitches():
    s, _ = sparse(np.uint16, (4,), x0=X0, y0=Y0, rows=ROWS)
    assert s.row_bytes == s.pitch_bytes == (PITCH + X0) * 8 and not s.packed and s.ptrs() == [s.ptr]
    assert s.ptr == s.dev.data_ptr() + GUARD + (Y0 * (PITCH + X0) + X0) * 8 == s.rows_view().data_ptr()
    p = gpu_kit.SparseSurface(W, H, np.uint16, content=np.arange(W * H, dtype=np.uint16), device="cpu")
    assert p.packed and p.pitch_bytes == 0 and p.row_bytes == 2 * W and p.nbytes == 2 * W * H and p.ptr == p.dev.data_ptr()
    texels, intact = p.read()
    assert intact and np.array_equal(texels, np.arange(W * H, dtype=np.uint16).reshape(H, W))
    f = gpu_kit.SparseSurface(W, H, np.uint8, pitch=PITCH, guard=GUARD, fill=0x00, device="cpu")       # another fill byte
    assert f.intact() and not f.texels().any()
    f.dev[GUARD + W] = gpu_kit.SENTINEL
    assert not f.intact()


@pytest.mark.parametrize("fmt,dtype,pattern", [(0, np.float32, [0x00, 0x00, 0xc0, 0x7f]), (1, np.uint16, [0xff, 0xff]),
                                               (2, np.uint32, [0xff] * 4), (3, np.uint16, [0x00, 0x7e])])
def test_depth_pad_words(fmt, dtype, pattern):
    from miniengineao_amd import _lib as L
    assert (L.DEPTH_F32, L.DEPTH_UNORM16, L.DEPTH_UNORM24, L.DEPTH_F16) == (0, 1, 2, 3)
    content = [np.full((H, W), 3, dtype)] * 2
    s = gpu_kit.Surface(W, H, dtype, n=2, pitch=PITCH, x0=X0, y0=Y0, rows=ROWS, guard=GUARD, pad_word=gpu_kit.DEPTH_PAD_WORD[fmt],
                        content=content, device=None)
    body = s.host[GUARD:-GUARD].copy()
    assert np.all(s.host[:GUARD] == gpu_kit.SENTINEL) and np.all(s.host[-GUARD:] == gpu_kit.SENTINEL)
    pad = np.ones((2, ROWS, PITCH), bool)
    pad[:, Y0:Y0 + H, X0:X0 + W] = False
    words = body.reshape(2, ROWS, PITCH, len(pattern))
    assert np.all(words[pad] == np.array(pattern, np.uint8)) and np.all(s.frames()[~pad] == 3)
    if fmt == 0:
        assert np.isnan(s.frames()[pad]).all()
    raw = s.host.copy()
    raw[GUARD + 1] ^= 0x80                                                         # the padding is checked whatever it holds
    assert s.intact(s.host) and not s.intact(raw)
