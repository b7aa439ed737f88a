"""The NumPy model of MEAO_COLOR_RGBA8_SRGB (tests/srgb_format.py) against the figures include/meao.h states for the format, and the
committed table include against the model: no device needed."""
import hashlib
import os
import re
import subprocess
import sys

import mpmath
import numpy as np

from tests import color_formats as CF
from tests import srgb_format as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "miniengineao_amd", "csrc", "meao_srgb_tables.inc")

D, T = S.tables()
CODES = np.arange(256, dtype=np.uint8)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def r8_products():
    """enc(D[c] * (a / 255)) indexed [c][a], the quotient rounded to f32."""
    f = CF.unorm8_to_f32(CODES)[None, :]
    return S.enc((S.dec(CODES)[:, None] * f).astype(np.float32))


def test_tables_have_the_stated_hashes_and_anchor_words():
    assert D.shape == (256,) and T.shape == (255,) and D.dtype == T.dtype == np.float32
    assert sha(D.astype("<f4")) == "48a8f05136456237aae2c5349e5f0199a182daa19b7c099eb542058f794b9c5b"
    assert sha(T.astype("<f4")) == "0b408a80ff623c35aef23dc30ed2669cc9893ecc3227e21394a963f4e5bb51de"
    assert sha(r8_products().astype(np.uint8)) == "c7ccee49d6fa41ef4c5a950ae2d9263efd487244dee3eeef6adbc3091ffb79df"
    dw, tw = D.view(np.uint32), T.view(np.uint32)
    assert [int(dw[k]) for k in (1, 10, 11, 128, 254)] == [0x399f22b4, 0x3b46eb61, 0x3b5b518e, 0x3e5d0a89, 0x3f7db8de]
    assert [int(tw[k - 1]) for k in (1, 10, 11, 128, 255)] == [0x391f22b4, 0x3b3cf936, 0x3b50f2d1, 0x3e5b2d9a, 0x3f7edc0e]
    assert D[0] == 0 and D[255] == 1


def test_tables_increase_and_the_encode_inverts_the_decode():
    assert np.all(np.diff(D) > 0) and np.all(np.diff(T) > 0)
    assert np.array_equal(S.enc(D), CODES)                       # a factor of exactly 1 leaves every texel untouched
    ones = np.ones((1, 256), np.float16).view(np.uint16)
    color = np.stack([CODES, CODES[::-1], CODES, CODES], axis=-1)[None]
    for mode in (S.MULTIPLY, S.AMBIENT_ONLY):
        assert np.array_equal(S.composite(ones, S.AO_F16, color, S.RGBA8_SRGB, mode)[0], color)


def test_thresholds_are_ceilings_not_nearest():
    with mpmath.workprec(S.BITS):
        for k in range(1, 256):
            b, t = S.boundary(k), T[k - 1]
            below = np.nextafter(t, np.float32(0))
            assert mpmath.mpf(float(t)) >= b > mpmath.mpf(float(below)), k
        nearest = sum(abs(mpmath.mpf(float(T[k - 1])) - S.boundary(k)) <= abs(mpmath.mpf(float(np.nextafter(T[k - 1], np.float32(0)))) - S.boundary(k))
                      for k in range(1, 256))
    assert 0 < nearest < 255                                     # a nearest-rounded table would differ: the distinction is real


def parse_inc(text):
    """-> (D words, T words): the hex words under each of the include's two block comments."""
    blocks = re.split(r"/\* ([DT])\[[^\]]*\][^*]*\*/", text)
    got = {blocks[i]: [int(w, 16) for w in re.findall(r"0x([0-9a-f]{8})u,", blocks[i + 1])] for i in range(1, len(blocks), 2)}
    return np.array(got["D"], np.uint32), np.array(got["T"], np.uint32)


def test_committed_include_holds_the_models_words():
    text = open(INC).read()
    d, t = parse_inc(text)
    assert np.array_equal(d, D.view(np.uint32)) and np.array_equal(t, T.view(np.uint32))
    assert len(re.findall(r"0x[0-9a-f]{8}u,", text)) == 511     # nothing else in the initializer list
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_srgb_tables.py"), "--check"], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr


def test_special_operands():
    f = np.float32
    nan = np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001], np.uint32).view(np.float32)
    assert np.all(S.enc(nan) == 0)
    assert np.all(S.enc(np.array([0.0, -0.0, -1e-30, -1.0, -np.inf], f)) == 0)
    assert np.all(S.enc(np.array([1e-45, 1e-40, 1.1754942e-38], f)) == 0)          # denormals lie below T[1]
    assert np.all(S.enc(np.array([1.0, 1.0000001, 2.0, 3e38, np.inf], f)) == 255)
    assert S.enc(T[0]) == 1 and S.enc(np.nextafter(T[0], f(0))) == 0
    assert S.enc(T[254]) == 255 and S.enc(np.nextafter(T[254], f(0))) == 254
    for k in (1, 10, 11, 128, 255):                              # across the joint of the two segments too
        assert S.enc(T[k - 1]) == k and S.enc(np.nextafter(T[k - 1], f(0))) == k - 1


def test_alpha_and_gbuffer0_move_as_in_rgba8():
    rng = np.random.default_rng(5)
    color = rng.integers(0, 256, (16, 16, 4), dtype=np.uint8)
    g0 = rng.integers(0, 256, (16, 16, 4), dtype=np.uint8)
    ao = rng.integers(0, 256, (16, 16), dtype=np.uint8)
    for mode in (S.MULTIPLY, S.AMBIENT_ONLY, S.DEBUG):
        c, g = S.composite(ao, S.AO_R8, color, S.RGBA8_SRGB, mode, g0)
        lc, lg = CF.composite(ao, CF.AO_R8, color, CF.RGBA8, mode, g0)
        assert np.array_equal(c[..., 3], lc[..., 3]) and np.array_equal(g, lg), mode
    assert np.array_equal(S.composite(ao, S.AO_R8, color, S.RGBA8_SRGB, S.AMBIENT_ONLY, g0)[0][..., 3], color[..., 3])
    assert np.array_equal(S.composite(ao, S.AO_R8, color, S.RGBA8_SRGB, S.MULTIPLY, g0)[1], g0)


def test_why_the_format_exists():
    """On an sRGB surface, multiplying the stored codes (MEAO_COLOR_RGBA8) differs from the blend in linear light in 59 777 of the
    65 536 (code, R8 AO) pairs, by up to 73 codes."""
    f = CF.unorm8_to_f32(CODES)[None, :]
    stored = CF.f32_to_unorm8((CF.unorm8_to_f32(CODES)[:, None] * f).astype(np.float32)).astype(np.int32)
    d = np.abs(r8_products().astype(np.int32) - stored)
    assert int((d > 0).sum()) == 59777 and int(d.max()) == 73
