"""The interface, checked once and completely: every function, struct, enum and #define of the header (tests/abi_model.py parses
it) against the ctypes mirror, the C++ wrapper, the never-compiled C# P/Invoke source, the built library and the committed
snapshot.  The second half proves the checker: one mutation at a time of a mirror or of the header text must give a finding that
names what was changed."""
import ctypes as C
import json
import subprocess
import types

import pytest

from miniengineao_amd import _lib as L
from tests import abi_model as A

MODEL = A.header_model()
STRUCTS = A.python_structs(L)
HPP = A.read(A.HPP_PATH)
CSHARP = A.read(A.CSHARP_PATH)

# What the C++ wrapper deliberately does not wrap, and why.  A header function is called in the wrapper or listed here, never both.
UNWRAPPED = {
    "meao_abi_version": "the wrapper is compiled against the header it calls: nothing to probe",
    "meao_level_dims": "host-plan query without a context: a C++ host calls the C function itself",
    "meao_zbuffer_params": "host-plan query",
    "meao_render_constants_for": "host-plan query",
    "meao_render_constants_variant": "host-plan query",
    "meao_upsample_constants_for": "host-plan query",
    "meao_describe_buffer": "host-plan query",
    "meao_algorithmic_bytes": "host-plan query",
    "meao_debug_set": "launch-structure overrides for tests and A/B runs: through native()",
    "meao_debug_view": "the reference's debug picture, for tests: through native()",
    "meao_set_profiling": "per-pass timing is what the tools measure, through the C calls",
    "meao_get_pass_times": "as meao_set_profiling",
    "meao_selftest": "device self-tests, run by the test suite",
    "meao_get_params": "reads back what the host itself set",
    "meao_get_config": "reads back what the host itself set",
    "meao_pool_context": "hands out a member's raw context: through native()",
    "meao_pool_composite_enqueue": "the pool class wraps the _pitched and _format enqueues, of which this is the pitch-0 RGBA16F form",
    "meao_pool_composite_flush": "a gap, not a decision: the pool class enqueues composites (CompositeWithNextFramePitched / Format) but "
                                 "offers no flush, so a batch that waits at destruction is discarded unless the host calls this on native()",
    "meao_pool_composite_pending": "the same gap: the context class has CompositePending(), the pool class has no counterpart",
    "meao_device_numa_node": "takes neither a context nor a pool: a C++ host calls the C function itself",
}

# The header enums MeaoNative.cs deliberately does not mirror, and why.  A header enum has its C# enum or is listed here, never both.
UNMIRRORED_ENUMS = {
    "meao_pass": "C# carries the pass count (NumPasses) and indexes the arrays of meao_algorithmic_bytes / meao_get_pass_times by number",
    "meao_pool_path": "the import of meao_pool_gather_path documents the three values in its comment; no C# caller branches on them",
    "meao_debug_key": "keys of meao_debug_set, launch-structure overrides for tests and A/B runs, which are driven from Python",
}


def none(findings):
    assert not findings, "\n" + "\n".join(findings)


def test_the_model_is_complete():
    assert (len(MODEL["functions"]), len(MODEL["structs"]), len(MODEL["enums"])) == (81, 7, 13)
    assert len(UNWRAPPED) == 20
    none(A.check_header_text(A.header_text()))


def test_the_interface_is_the_committed_snapshot():
    with open(A.SNAPSHOT_PATH) as f:
        none(A.check_snapshot(MODEL, json.load(f)))
    assert A.read(A.SNAPSHOT_PATH) == A.dump(MODEL)


def test_ctypes_signatures():
    none(A.check_ctypes_signatures(MODEL, L.SIGNATURES, STRUCTS))


def test_ctypes_structs_have_the_compilers_layout():
    none(A.check_ctypes_structs(MODEL, STRUCTS, A.compiler_layout()))


def test_python_enums_and_constants():
    none(A.check_python_constants(MODEL, L))


def test_csharp_imports():
    none(A.check_csharp_imports(MODEL, A.parse_csharp(CSHARP)))


def test_csharp_structs():
    none(A.check_csharp_structs(MODEL, A.parse_csharp(CSHARP)))


def test_csharp_enums_and_constants():
    none(A.check_csharp_enums_and_constants(MODEL, A.parse_csharp(CSHARP), UNMIRRORED_ENUMS))


def test_cpp_wrapper_calls_everything_it_does_not_exempt():
    none(A.check_hpp(MODEL, HPP, UNWRAPPED))


def test_library_exports_the_interface_and_nothing_of_the_tests(meao_lib):
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    none(A.check_exports(MODEL, nm))
    assert meao_lib.meao_abi_version() == MODEL["defines"]["MEAO_ABI_VERSION"]
    assert not hasattr(meao_lib, "meao_test_counters")


# ---- the checker, proved: each mutation must be reported, by the name of what it changed ------------------------------------------

def header_with(old, new, count=1):
    assert A.header_text().count(old) >= count, old
    return A.header_text().replace(old, new, count)


def csharp_with(old, new):
    assert CSHARP.count(old) == 1, old
    return A.parse_csharp(CSHARP.replace(old, new))


def csharp_enums_with(old, new):
    return csharp_with(old, new), UNMIRRORED_ENUMS


def signatures_with(name, value):
    return dict({k: v for k, v in L.SIGNATURES.items() if k != name}, **({name: value} if value else {}))


def swapped_extent():
    class Extent(C.Structure):
        _fields_ = [("height", C.c_int32), ("width", C.c_int32), ("depth_pitch", C.c_uint64), ("ao_pitch", C.c_uint64)]
    return dict(STRUCTS, meao_extent=Extent)


def narrowed_extent():
    class Extent(C.Structure):
        _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("depth_pitch", C.c_uint32), ("ao_pitch", C.c_uint64)]
    return dict(STRUCTS, meao_extent=Extent)


def lib_with(**changed):
    return types.SimpleNamespace(**dict({k: v for k, v in vars(L).items() if k.isupper()}, **changed))


PITCHED_AS_INT = "const void *const *depth, int32_t depth_pitch, int32_t depth_loc"
SWAPPED_HEADER = ("typedef struct meao_extent {\n    int32_t width, height;", "typedef struct meao_extent {\n    int32_t height, width;")
BATCH_PARAMS = "meao_prefetch_batch_params(IntPtr ctx, int n, IntPtr[] depth, [In] MeaoParams[] prm);"
_sig = L.SIGNATURES["meao_reserve_bytes"]

MUTATIONS = {
    # id: (findings, the name a finding must carry)
    "header argument type, seen by ctypes": (lambda: A.check_ctypes_signatures(
        A.parse_header(header_with("const void *const *depth, uint64_t depth_pitch, int32_t depth_loc", PITCHED_AS_INT)),
        L.SIGNATURES, STRUCTS), "meao_execute_batch_pitched"),
    "header argument type, seen by C#": (lambda: A.check_csharp_imports(
        A.parse_header(header_with("const void *const *depth, uint64_t depth_pitch, int32_t depth_loc", PITCHED_AS_INT)),
        A.parse_csharp(CSHARP)), "meao_execute_batch_pitched"),
    "header argument type, seen by the snapshot": (lambda: A.check_snapshot(
        A.parse_header(header_with("const void *const *depth, uint64_t depth_pitch, int32_t depth_loc", PITCHED_AS_INT)),
        json.loads(A.read(A.SNAPSHOT_PATH))), "meao_execute_batch_pitched"),
    "C# argument dropped": (lambda: A.check_csharp_imports(MODEL, csharp_with(
        "meao_resize(IntPtr ctx, int width, int height)", "meao_resize(IntPtr ctx, int width)")), "meao_resize"),
    "C# ulong -> int": (lambda: A.check_csharp_imports(MODEL, csharp_with(
        "meao_prefetch_batch_pitched(IntPtr ctx, int n, IntPtr[] depth, ulong depth_pitch",
        "meao_prefetch_batch_pitched(IntPtr ctx, int n, IntPtr[] depth, int depth_pitch")), "meao_prefetch_batch_pitched"),
    "C# [In] MeaoParams[] -> IntPtr": (lambda: A.check_csharp_imports(MODEL, csharp_with(
        BATCH_PARAMS, BATCH_PARAMS.replace("[In] MeaoParams[]", "IntPtr"))), "meao_prefetch_batch_params"),
    "C# parameter renamed": (lambda: A.check_csharp_imports(MODEL, csharp_with(
        "meao_reserve(IntPtr ctx, int max_width,", "meao_reserve(IntPtr ctx, int width,")), "meao_reserve: parameter max_width"),
    "C# return type": (lambda: A.check_csharp_imports(MODEL, csharp_with(
        "extern IntPtr meao_pool_context(", "extern int meao_pool_context(")), "meao_pool_context"),
    "C# library name": (lambda: A.check_csharp_imports(MODEL, csharp_with('Lib = "meao_hip"', 'Lib = "meao"')), "meao_hip"),
    "SIGNATURES argtype at equal count": (lambda: A.check_ctypes_signatures(MODEL, signatures_with(
        "meao_reserve_bytes", (_sig[0], _sig[1][:3] + [C.POINTER(C.c_int32)])), STRUCTS), "meao_reserve_bytes: argument 3"),
    "SIGNATURES restype": (lambda: A.check_ctypes_signatures(MODEL, signatures_with(
        "meao_last_error", (C.c_void_p, L.SIGNATURES["meao_last_error"][1])), STRUCTS), "meao_last_error: the return type"),
    "struct fields swapped in the header, seen by ctypes": (lambda: A.check_ctypes_structs(
        A.parse_header(header_with(*SWAPPED_HEADER)), STRUCTS, A.compiler_layout(header_with(*SWAPPED_HEADER))), "meao_extent"),
    "struct fields swapped in the header, seen by C#": (lambda: A.check_csharp_structs(
        A.parse_header(header_with(*SWAPPED_HEADER)), A.parse_csharp(CSHARP)), "meao_extent"),
    "struct fields swapped in ctypes": (lambda: A.check_ctypes_structs(MODEL, swapped_extent(), A.compiler_layout()), "meao_extent"),
    "struct field narrowed in ctypes": (lambda: A.check_ctypes_structs(MODEL, narrowed_extent(), A.compiler_layout()),
                                        "meao_extent.depth_pitch"),
    "struct fields swapped in C#": (lambda: A.check_csharp_structs(MODEL, csharp_with(
        "public ulong ao_pitch;\n        public ulong color_pitch;", "public ulong color_pitch;\n        public ulong ao_pitch;")),
        "meao_target_extent"),
    "C# struct field type": (lambda: A.check_csharp_structs(MODEL, csharp_with(
        "public ulong bytes;", "public uint bytes;")), "meao_desc.bytes"),
    "C# struct array extent": (lambda: A.check_csharp_structs(MODEL, csharp_with(
        "SizeConst = 2)] public float[] inv_slice_dimension", "SizeConst = 4)] public float[] inv_slice_dimension")),
        "meao_render_constants.inv_slice_dimension"),
    "C# struct not sequential": (lambda: A.check_csharp_structs(MODEL, csharp_with(
        "[StructLayout(LayoutKind.Sequential)]\n    public struct MeaoDesc", "[StructLayout(LayoutKind.Auto)]\n    public struct MeaoDesc")),
        "meao_desc"),
    "C# enum value": (lambda: A.check_csharp_enums_and_constants(MODEL, *csharp_enums_with("Rgba8Srgb = 5", "Rgba8Srgb = 4")), "MeaoColorFormat: member Rgba8Srgb"),
    "C# enum member missing": (lambda: A.check_csharp_enums_and_constants(MODEL, *csharp_enums_with(", LinearF16 = 5", "")), "MeaoDepthFormat: member MEAO_DEPTH_LINEAR_F16"),
    "C# enum deleted": (lambda: A.check_csharp_enums_and_constants(MODEL, *csharp_enums_with(
        "    public enum MeaoMem { Host = 0, Device = 1 }\n", "")), "meao_mem"),
    "C# enum the list says is unmirrored": (lambda: A.check_csharp_enums_and_constants(
        MODEL, A.parse_csharp(CSHARP), dict(UNMIRRORED_ENUMS, meao_mem="")), "meao_mem"),
    "unmirrored enum the header does not have": (lambda: A.check_csharp_enums_and_constants(
        MODEL, A.parse_csharp(CSHARP), dict(UNMIRRORED_ENUMS, meao_gone="")), "meao_gone"),
    "header enum neither in C# nor listed": (lambda: A.check_csharp_enums_and_constants(
        MODEL, A.parse_csharp(CSHARP), {k: v for k, v in UNMIRRORED_ENUMS.items() if k != "meao_pool_path"}), "meao_pool_path"),
    "_lib enum value": (lambda: A.check_python_constants(MODEL, lib_with(COLOR_RGBA8_SRGB=4)), "MEAO_COLOR_RGBA8_SRGB"),
    "_lib pass order": (lambda: A.check_python_constants(MODEL, lib_with(
        PASS_NAMES=L.PASS_NAMES[:5] + L.PASS_NAMES[:4:-1])), "meao_pass"),
    "_lib ABI version stale": (lambda: A.check_python_constants(MODEL, lib_with(ABI_VERSION=6)), "MEAO_ABI_VERSION"),
    "C# AbiVersion stale": (lambda: A.check_csharp_enums_and_constants(MODEL, *csharp_enums_with(
        "AbiVersion = %d;" % MODEL["defines"]["MEAO_ABI_VERSION"], "AbiVersion = 6;")), "AbiVersion"),
    "function missing from C#": (lambda: A.check_csharp_imports(MODEL, csharp_with(
        "[DllImport(Lib)] public static extern int meao_pool_synchronize(IntPtr pool);", "")), "meao_pool_synchronize"),
    "function missing from SIGNATURES": (lambda: A.check_ctypes_signatures(MODEL, signatures_with("meao_synchronize", None), STRUCTS),
                                         "meao_synchronize"),
    "function neither in the wrapper nor exempt": (lambda: A.check_hpp(MODEL, HPP.replace("meao_hostile_frames(", "hostile_frames("),
                                                                       UNWRAPPED), "meao_hostile_frames"),
    "function only named in a comment of the wrapper": (lambda: A.check_hpp(MODEL, HPP.replace(
        "check(meao_hostile_frames(", "// meao_hostile_frames(ctx_, &mask) was here\n        check(hostile_frames("), UNWRAPPED),
        "meao_hostile_frames"),
    "exempt function that the wrapper calls": (lambda: A.check_hpp(MODEL, HPP, dict(UNWRAPPED, meao_resize="")), "meao_resize"),
    "function not exported": (lambda: A.check_exports(MODEL, "".join(
        "0 T %s\n" % n for n in MODEL["functions"] if n != "meao_reserve")), "meao_reserve"),
    "test hook exported": (lambda: A.check_exports(MODEL, "".join(
        "0 T %s\n" % n for n in list(MODEL["functions"]) + ["meao_test_counters"])), "meao_test_counters"),
    "test hook in the header": (lambda: A.check_header_text(header_with(
        "MEAO_API int32_t meao_abi_version(void);", "MEAO_API int32_t meao_test_counters(void);")), "meao_test_counters"),
    "const struct pointer without a row": (lambda: A.check_csharp_imports(A.parse_header(header_with(
        "meao_get_config(const meao_ctx *ctx, meao_config *out)", "meao_get_config(const meao_ctx *ctx, const meao_desc *out)")),
        A.parse_csharp(CSHARP)), "meao_get_config: no C# row for the C type 'const meao_desc *'"),
    "C type without a row": (lambda: A.check_csharp_imports(A.parse_header(header_with(
        "meao_selftest(meao_ctx *ctx, int32_t which", "meao_selftest(meao_ctx *ctx, int16_t which")), A.parse_csharp(CSHARP)),
        "meao_selftest: no C# row for the C type 'int16_t'"),
}


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_a_mutation_is_reported_by_name(mutation):
    findings, name = MUTATIONS[mutation][0](), MUTATIONS[mutation][1]
    assert findings and all(name in f for f in findings), (mutation, findings)


def test_the_unmutated_inputs_of_the_mutations_are_clean():
    """The copies the mutations start from give no finding: what a mutation reports is the mutation."""
    none(A.check_ctypes_signatures(MODEL, signatures_with("meao_abi_version", L.SIGNATURES["meao_abi_version"]), STRUCTS))
    none(A.check_python_constants(MODEL, lib_with()))
    none(A.check_exports(MODEL, "".join("0 T %s\n" % n for n in MODEL["functions"])))
    none(A.check_snapshot(A.parse_header(A.header_text()), json.loads(A.dump(MODEL))))
