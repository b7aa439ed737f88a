"""Writes miniengineao_amd/csrc/meao_srgb_tables.inc: the two f32 tables that define MEAO_COLOR_RGBA8_SRGB (include/meao.h).

    python tools/gen_srgb_tables.py            # (re)writes the include
    python tools/gen_srgb_tables.py --check    # exit status 1 if the committed include differs from what would be written

D[k], k = 0..255: the f32 nearest to lin(k / 255); T[k], k = 1..255: the smallest f32 >= lin((k - 0.5) / 255), with
lin(s) = s / 12.92 for s <= 0.04045 and ((s + 0.055) / 1.055)^2.4 otherwise (IEC 61966-2-1).  Computed with mpmath at 256 bits;
neither table has a value within 2^-30 (relative) of an f32 rounding boundary, so any arithmetic of 100 bits or more gives the
same words.  The include is a C initializer list: 256 words of D, then 255 words of T[1..255], eight per line, each block under a
comment line of its own."""
import os
import struct
import sys

import mpmath

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "miniengineao_amd", "csrc", "meao_srgb_tables.inc")
BITS = 256


def lin(s):
    s = mpmath.mpf(s)
    if s <= mpmath.mpf("0.04045"):
        return s / mpmath.mpf("12.92")
    return ((s + mpmath.mpf("0.055")) / mpmath.mpf("1.055")) ** mpmath.mpf("2.4")


def f32_word(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def f32_of(word):
    return struct.unpack("<f", struct.pack("<I", word))[0]


def nearest_f32(v):
    """The f32 word nearest to the positive real v (a tie would raise: there is none in these tables)."""
    lo = f32_word(float(v))                       # the double nearest to v, rounded to f32: within one f32 step of the answer
    best = None
    for w in (lo - 1, lo, lo + 1):
        if w < 0:
            continue
        d = abs(mpmath.mpf(f32_of(w)) - v)
        if best is None or d < best[0]:
            best = (d, w)
        elif d == best[0]:
            raise ValueError("tie")
    return best[1]


def ceil_f32(v):
    """The word of the smallest f32 >= the positive real v."""
    w = nearest_f32(v)
    while mpmath.mpf(f32_of(w)) < v:
        w += 1
    while w > 0 and mpmath.mpf(f32_of(w - 1)) >= v:
        w -= 1
    return w


def tables():
    """-> (D words [256], T words [255] for k = 1..255)."""
    with mpmath.workprec(BITS):
        d = [0] + [nearest_f32(lin(mpmath.mpf(k) / 255)) for k in range(1, 256)]
        t = [ceil_f32(lin((mpmath.mpf(k) - mpmath.mpf("0.5")) / 255)) for k in range(1, 256)]
    return d, t


def render(d, t):
    def block(words):
        return "".join("    " + " ".join(f"0x{w:08x}u," for w in words[i:i + 8]) + "\n" for i in range(0, len(words), 8))
    return ("/* meao_srgb_tables.inc -- written by tools/gen_srgb_tables.py, not by hand.  The f32 words that define\n"
            "   MEAO_COLOR_RGBA8_SRGB (include/meao.h): an initializer list of 256 + 255 words. */\n"
            "/* D[0..255]: the f32 nearest to lin(k / 255) */\n" + block(d) +
            "/* T[1..255]: the smallest f32 >= lin((k - 0.5) / 255) */\n" + block(t))


def main() -> int:
    text = render(*tables())
    if "--check" in sys.argv[1:]:
        same = os.path.exists(INC) and open(INC).read() == text
        print(f"{os.path.relpath(INC, ROOT)}: {'up to date' if same else 'DIFFERS from the generated tables'}")
        return 0 if same else 1
    with open(INC, "w") as fh:
        fh.write(text)
    print(os.path.relpath(INC, ROOT))
    return 0


if __name__ == "__main__":
    sys.exit(main())
