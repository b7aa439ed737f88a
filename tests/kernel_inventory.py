"""The kernel instantiations of the loaded libmeao_hip.so (miniengineao_amd._lib.LIB_PATH: MEAO_LIB_PATH respected), by short name.

Every kernel of the library's gfx950 code objects has a kernel descriptor symbol `<mangled name>.kd` in its .hip_fatbin section
(codehash.fatbin_bytes).  The mangled names are demangled with c++filt and shortened the way tools/kernel_resources.py prints them:
`render_kernel<0, false, 1, true>`.  normalise() maps a rocprofv3 Kernel_Name, mangled or demangled, to the same text, so that a
kernel trace can be checked against this list (tests/test_kernel_coverage_gpu.py)."""
from __future__ import annotations

import functools
import importlib.util
import os
import re
import subprocess

from miniengineao_amd import codehash

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the six (AOFMT, RTNE, DIV) columns a context can run (tools/kernel_instantiations.py): RTNE storage divides with IEEE only
COLUMNS = (("0", "false", "0"), ("0", "false", "1"), ("0", "true", "1"),
           ("1", "false", "0"), ("1", "false", "1"), ("1", "true", "1"))

# kernel (R8, RTZ, exact division = what bench.py times): (waves per SIMD, max VGPRs, max LDS bytes per workgroup)
HOT = {
    "render_kernel<0, false, 0, false>": (8, 64, 40960),                                   # 4 workgroups of 8 waves per CU
    "render_with_composite_kernel<0, false, 0>": (8, 64, 40960),
    "upsample_final_kernel<0, false, 0, true>": (7, 72, 163840 // 7),                       # seven 256-thread workgroups per CU
    "upsample_final_with_next_downsample_kernel<0, false, 0>": (7, 72, 163840 // 7),
    "upsample_kernel<0, false, 0>": (8, 64, 163840 // 8),
    "upsample_two_level_kernel<0, false, 0>": (8, 64, 163840 // 8),                       # compiled for 8 waves per SIMD: 4080 workgroups = 1.99 rounds of the slots
    "downsample_kernel<true, 0, 2>": (8, 64, 0),
}


@functools.lru_cache(maxsize=None)
def _short():
    spec = importlib.util.spec_from_file_location("_meao_kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.short


def demangle(names):
    names = list(names)
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(names), "c++filt returned %d names for %d" % (len(out), len(names))
    return out


@functools.lru_cache(maxsize=None)
def mangled_names(lib_path=None) -> tuple:
    """Sorted mangled names of every kernel in the library's device code."""
    if lib_path is None:
        from miniengineao_amd import _lib
        lib_path = _lib.LIB_PATH
    blob = codehash.fatbin_bytes(lib_path)
    return tuple(sorted({m.decode()[:-3] for m in re.findall(rb"_ZN4meao\w+\.kd", blob)}))


@functools.lru_cache(maxsize=None)
def instantiations(lib_path=None) -> tuple:
    """Sorted short names of every kernel in the library's device code."""
    return tuple(sorted(_short()(n) for n in demangle(mangled_names(lib_path))))


def normalise(kernel_names):
    """Short names of the meao kernels among trace names (rocprofv3 prints them demangled or mangled); other kernels dropped."""
    names = [n.strip() for n in kernel_names]
    names = [n for n in names if n.startswith("_ZN4meao") or "meao::" in n]
    mangled = [re.sub(r"\.kd$", "", n.split()[0]) if n.startswith("_ZN4meao") else n for n in names]
    todo = sorted({n for n in mangled if n.startswith("_ZN4meao")})
    done = dict(zip(todo, demangle(todo))) if todo else {}
    return [_short()(done.get(n, n)) for n in mangled]


def split(name):
    """'render_kernel<0, false, 1, true>' -> ('render_kernel', ['0', 'false', '1', 'true'])"""
    m = re.match(r"(\w+)<(.*)>$", name)
    return (m.group(1), [a.strip() for a in m.group(2).split(",")]) if m else (name, [])


def column_of(name):
    """The (AOFMT, RTNE, DIV) column of a render / upsample instantiation, ("ds", DIV) of a downsample one, None otherwise."""
    base, args = split(name)
    if base.startswith(("render", "upsample")) and len(args) >= 3:
        return tuple(args[:3])
    if base.startswith("downsample") and len(args) >= 2:
        return ("ds", args[1])
    return None
