"""tests/color_formats.py, the NumPy model the composite's other colour formats are tested against: known answers of the small
float conversions, and the model against the oracle where the two overlap (UNORM8 times AO is what the oracle does to GBuffer0.a)."""
import numpy as np
import pytest

from tests import color_formats as CF


def f32(x):
    return np.array([x], np.float32)


def below(x):
    return np.nextafter(np.float32(x), np.float32(0))


@pytest.mark.parametrize("value,m6,m5", [
    (1.0, 0x3C0, 0x1E0),
    (2.0 ** -20, 0x001, None), (2.0 ** -21, 0x000, 0x000),            # the smallest M = 6 subnormal; half of it ties to even (0)
    (-0.0, 0, 0), (-1.0, 0, 0), (-np.inf, 0, 0), (np.inf, 0x7C0, 0x3E0), (np.nan, 0x7FF, 0x3FF), (-np.nan, 0x7FF, 0x3FF),
    (1 + 2.0 ** -7, 0x3C0, None), (1 + 3 * 2.0 ** -7, 0x3C2, None),   # ties to even, both ways
    (65024.0, 0x7BF, 0x3E0), (64512.0, None, 0x3DF),                  # the largest finite codes (65024 is M = 5's halfway value)
    (65280.0, 0x7C0, 0x3E0),                                          # M = 6's halfway value -> +inf
])
def test_enc_known_answers(value, m6, m5):
    if m6 is not None:
        assert CF.enc(f32(value), 6)[0] == m6
    if m5 is not None:
        assert CF.enc(f32(value), 5)[0] == m5


def test_just_below_the_halfway_values_is_the_largest_finite_code():
    assert CF.enc(f32(below(65280.0)), 6)[0] == 0x7BF
    assert CF.enc(f32(below(65024.0)), 5)[0] == 0x3DF


@pytest.mark.parametrize("M", [6, 5])
def test_every_code_is_its_f16_value_and_round_trips(M):
    codes = np.arange(32 << M, dtype=np.uint32)
    got = CF.dec(codes, M)
    via_f16 = (codes << (10 - M)).astype(np.uint16).view(np.float16).astype(np.float32)
    assert np.array_equal(got.view(np.uint32)[~np.isnan(via_f16)], via_f16.view(np.uint32)[~np.isnan(via_f16)])
    assert np.array_equal(np.isnan(got), np.isnan(via_f16))
    assert np.isnan(got).sum() == (1 << M) - 1 and np.isinf(got).sum() == 1
    ok = ~np.isnan(got)
    assert np.array_equal(CF.enc(got, M)[ok], codes[ok])
    assert (CF.enc(got, M)[~ok] == (32 << M) - 1).all()


@pytest.mark.parametrize("M", [6, 5])
def test_enc_rounds_to_the_nearest_code(M):
    """Random f32 values in range: the code's value and its neighbours' bracket the input, and the chosen one is nearest."""
    rng = np.random.default_rng(M)
    x = np.ldexp(rng.random(200000) + 1.0, rng.integers(-24, 17, 200000)).astype(np.float32)
    c = CF.enc(x, M).astype(np.int64)
    v = CF.dec(c, M).astype(np.float64)
    lo, hi = CF.dec(np.maximum(c - 1, 0), M).astype(np.float64), CF.dec(np.minimum(c + 1, 31 << M), M).astype(np.float64)
    finite = c < (31 << M)
    err = np.abs(v - x)[finite]
    assert (err <= np.abs(lo - x)[finite]).all() and (err <= np.abs(hi - x)[finite]).all()
    top = float(CF.dec((31 << M) - 1, M)) + 2.0 ** (14 - M)               # the halfway value to 2^16
    assert (x[~finite] >= top).all() and (x[finite] < top).all()


def test_rgba8_ambient_only_is_what_the_oracle_does_to_gbuffer0_alpha(oracle):
    """All 256 x 256 (code, R8 AO) pairs: a colour channel times keep in the model, GBuffer0.a in oracle.composite."""
    code, ao = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8))
    color = np.repeat(code[..., None], 4, axis=2)
    want_c, want_g = CF.composite(ao, CF.AO_R8, color, CF.RGBA8, CF.AMBIENT_ONLY, color)
    g = color.copy()
    oracle.composite(np.ascontiguousarray(ao), np.zeros((256, 256, 4), np.uint16), 1, 0, g)
    assert np.array_equal(want_g, g)
    for k in range(3):
        assert np.array_equal(want_c[..., k], g[..., 3])
    assert np.array_equal(want_c[..., 3], code) and np.array_equal(g[..., :3], color[..., :3])


def test_rgba32f_keeps_the_sign_of_a_zero_product():
    c = np.array([[[-0.0, 0.0, -1.0, -0.0]]], np.float32)
    got, _ = CF.composite(np.array([[128]], np.uint8), CF.AO_R8, c, CF.RGBA32F, CF.MULTIPLY)
    assert np.array_equal(np.signbit(got), [[[True, False, True, True]]])
