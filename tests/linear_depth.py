"""Linear view-space depth frames for the GPU suites: the Linearize of a raw frame, evaluated as the oracle evaluates it.

A raw frame d and its camera (far_clip a power of two); dist = Linearize(d) = 1 / fmaf(zp.x, d, zp.y) with the sky select, fmaf exact,
in C; z = dist * far (exact).  Then library(LINEAR, z) == oracle(d) bit for bit (tests/test_linear_depth_gpu.py)."""
import ctypes as C
import os
import subprocess

import numpy as np

_lin = []


def build_linearize(directory):
    """Linearize exactly as the oracle evaluates it (fmaf of the C library: exact whatever the compiler flags)."""
    src, lib = os.path.join(directory, "lin.c"), os.path.join(directory, "liblin.so")
    with open(src, "w") as f:
        f.write(r"""
#include <math.h>
#include <stddef.h>
void linearize(const float *d, float *out, size_t n, float zp0, float zp1, float sky)
{
    for (size_t i = 0; i < n; i++) out[i] = d[i] == sky ? 1e5f : 1.0f / fmaf(zp0, d[i], zp1);
}
""")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", lib, "-lm"], check=True)
    so = C.CDLL(lib)
    so.linearize.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_float, C.c_float, C.c_float]
    return so


def linearize():
    """build_linearize, once per process, in a temporary directory."""
    if not _lin:
        import tempfile
        _lin.append(build_linearize(tempfile.mkdtemp()))
    return _lin[0]


def to_linear(lin_c, d, cam, far=None):
    """(d with far-plane-or-beyond texels made sky, z) for raw f32 frame d of camera cam; z in the units of `far`."""
    far = np.float32(cam.far if far is None else far)
    fpn = np.float32(cam.far) / np.float32(cam.near)
    zp0, zp1 = ((fpn - np.float32(1), np.float32(1)) if cam.reversed_z else (np.float32(1) - fpn, fpn))
    sky = np.float32(0.0 if cam.reversed_z else 1.0)
    d = np.ascontiguousarray(d, np.float32).copy()
    dist = np.empty_like(d)
    lin_c.linearize(d.ctypes.data, dist.ctypes.data, d.size, float(zp0), float(zp1), float(sky))
    with np.errstate(invalid="ignore"):
        beyond = (dist >= 1) & (d != sky)
    d[beyond] = sky
    is_sky = d == sky
    with np.errstate(over="ignore", invalid="ignore"):
        z = dist * far
    alt = (np.arange(d.size).reshape(d.shape) & 1) == 1
    z[is_sky & alt] = np.inf
    z[is_sky & ~alt] = far
    return d, z.astype(np.float32)
