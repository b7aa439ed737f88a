"""One parsed model of the C header (the interface's single source of truth) and the checks of its three hand-written mirrors:
miniengineao_amd/_lib.py (ctypes), the C++ wrapper and bindings/csharp/MeaoNative.cs (never compiled: text checks are its only
guard).  Plain `re`, no compiler front end.  Every check takes the model and a mirror's text or object and returns a list of
findings, each naming the function, struct or field; tests/test_abi_mirrors.py asserts the lists are empty and proves each check
with a mutation.  tests/abi_snapshot.json pins the model: `python -m tests.abi_model --write-snapshot` regenerates it, so a change
of the interface shows as a diff of that file."""
import ctypes as C
import functools
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_PATH = os.path.join(ROOT, "include", "meao.h")
HPP_PATH = os.path.join(ROOT, "include", "meao.hpp")
CSHARP_PATH = os.path.join(ROOT, "bindings", "csharp", "MeaoNative.cs")
SNAPSHOT_PATH = os.path.join(ROOT, "tests", "abi_snapshot.json")


def read(path):
    with open(path) as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def header_text():
    """The header as written, comments included (for the tests that look for a contract's wording)."""
    return read(HEADER_PATH)


@functools.lru_cache(maxsize=None)
def header_prose():
    """The header with line breaks, indentation and the ' * ' that opens a comment's continuation line folded into single spaces:
    what a test searches for the wording of a contract, wherever the lines happen to break."""
    return " ".join(re.sub(r"\n\s*\*(?!/)", " ", header_text()).split())


# ---- the header ---------------------------------------------------------------------------------------------------------------

def _strip_comments(text):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))


def _ctype(text):
    """'const  void * const*' -> 'const void *const *': one spelling per C type."""
    return re.sub(r"\s*(\*+)\s*", r" \1", re.sub(r"\*\s+(?=\*)", "*", " ".join(text.split()))).strip()


def _declarator(decl, defines):
    """'const void *const *depth' -> ('const void *const *', 'depth', None); 'float out[4]' -> ('float', 'out', 4)."""
    m = re.fullmatch(r"(.*?)(\w+)\s*(?:\[\s*(\w+)\s*\])?", decl.strip(), re.S)
    extent = m.group(3)
    if extent is not None:
        extent = defines[extent] if extent in defines else int(extent, 0)
    return [_ctype(m.group(1)), m.group(2), extent]


def parse_header(text):
    """{"defines": {name: int}, "enums": {enum: {member: int}}, "structs": {struct: [[type, field, extent]]},
    "functions": {name: {"returns": type, "params": [[type, name, extent]]}}} of a header's text."""
    text = _strip_comments(text)
    defines = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(-?\w+)[ \t]*$", text, re.M)
               if re.fullmatch(r"-?(0[xX][0-9a-fA-F]+|\d+)", m.group(2))}
    enums = {}
    for m in re.finditer(r"typedef\s+enum\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", text, re.S):
        members, value = {}, -1
        for item in filter(None, (i.strip() for i in m.group(2).split(","))):
            name, _, expr = (p.strip() for p in item.partition("="))
            value = value + 1 if not expr else members[expr] if expr in members else defines[expr] if expr in defines else int(expr, 0)
            members[name] = value
        enums[m.group(1)] = members
    structs = {}
    for m in re.finditer(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", text, re.S):
        fields = []
        for decl in filter(None, (d.strip() for d in m.group(2).split(";"))):
            first, *more = decl.split(",")
            ctype, name, extent = _declarator(first, defines)
            fields.append([ctype, name, extent])
            fields += [[ctype] + _declarator(d, defines)[1:] for d in more]       # 'int32_t width, height;'
        structs[m.group(1)] = fields
    functions = {}
    for m in re.finditer(r"\bMEAO_API\s+([^;()]*?)\b(meao_\w+)\s*\(([^()]*)\)\s*;", text, re.S):
        params = [] if m.group(3).strip() == "void" else [_declarator(p, defines) for p in m.group(3).split(",")]
        functions[m.group(2)] = {"returns": _ctype(m.group(1)), "params": params}
    return {"defines": defines, "enums": enums, "structs": structs, "functions": functions}


@functools.lru_cache(maxsize=None)
def header_model():
    return parse_header(header_text())


def prototype(name):
    """['meao_ctx *ctx', 'int32_t n', ...]: the parameters of a header function as C writes them, for a feature's test that needs
    to say where its arguments sit."""
    return ["%s%s%s%s" % (t, "" if t.endswith("*") else " ", n, "[%d]" % e if e else "") for t, n, e in header_model()["functions"][name]["params"]]


def check_header_text(text):
    """Test hooks and oracle code are no part of the product's interface."""
    return ["the header names %s" % w for w in sorted(set(re.findall(r"\bmeao_(?:test_|oracle)\w*", text)))]


def dump(model):
    """The snapshot's text: one line per function, struct, enum and #define, so that a change reads as a diff of that line."""
    kinds = ["{\n%s\n }" % ",\n".join("  %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in model[kind].items()) for kind in sorted(model)]
    return "{\n%s\n}\n" % ",\n".join(" %s: %s" % (json.dumps(kind), body) for kind, body in zip(sorted(model), kinds))


def check_snapshot(model, snapshot):
    """The model against the committed pin, entry by entry."""
    out = []
    for kind in sorted(set(model) | set(snapshot)):
        have, want = model.get(kind, {}), snapshot.get(kind, {})
        out += ["%s %s: the header has %s, tests/abi_snapshot.json %s" % (kind, k, json.dumps(have.get(k)), json.dumps(want.get(k)))
                for k in sorted(set(have) | set(want)) if have.get(k) != want.get(k)]
    return out


# ---- names ----------------------------------------------------------------------------------------------------------------------

def camel(cname):
    """meao_target_extent -> TargetExtent: the struct's name in _lib.py; with 'Meao' in front, its name in C#."""
    return "".join(w.capitalize() for w in cname.split("_")[1:])


def fold(name):
    """CamelCase <-> UPPER_SNAKE, written once: both sides compare as their letters and digits in lower case."""
    return name.replace("_", "").lower()


def _enum_prefix(members):
    """The words every member of an enum starts with (MEAO_COLOR_ for meao_color_format; MEAO_ alone for meao_status, whose
    members are MEAO_OK and MEAO_ERR_*)."""
    words = [m.split("_") for m in members]
    n = 0
    while all(len(w) > n + 1 for w in words) and len({w[n] for w in words}) == 1:
        n += 1
    return "_".join(words[0][:n]) + "_"


# ---- C type -> ctypes type ------------------------------------------------------------------------------------------------------

SCALARS = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "float": C.c_float}
OPAQUE = {"meao_ctx *", "const meao_ctx *", "meao_pool *", "const meao_pool *", "meao_stream", "void *", "const void *"}
HANDLE_OUT = {"meao_ctx **", "meao_pool **"}
POINTER_ARRAYS = {"const void *const *", "void *const *"}


def _struct_pointer(model, ctype):
    """('meao_params', True) for 'const meao_params *'; None for anything that is no pointer to one of the header's structs."""
    m = re.fullmatch(r"(const )?(\w+) \*", ctype)
    return (m.group(2), bool(m.group(1))) if m and m.group(2) in model["structs"] else None


def ctypes_image(model, structs, ctype, extent=None, returned=False):
    """The ctypes type _lib.SIGNATURES must hold for a C parameter (or return) type; KeyError for a type without a row."""
    if returned and ctype == "void":
        return None                                             # return void            -> None
    if returned and ctype == "const char *":
        return C.c_char_p                                       # return const char *    -> c_char_p (a static string)
    if extent is not None:
        return C.POINTER(SCALARS[ctype] * extent)               # float x[4]             -> POINTER(c_float * 4)
    if ctype in SCALARS:
        return SCALARS[ctype]                                   # int32_t, uint64_t, ... -> c_int32, c_uint64, ...
    if ctype in OPAQUE:
        return C.c_void_p                                       # handles, void pointers -> c_void_p
    if ctype in HANDLE_OUT or ctype in POINTER_ARRAYS:
        return C.POINTER(C.c_void_p)                            # meao_ctx **, const void *const * -> POINTER(c_void_p)
    if _struct_pointer(model, ctype):
        return C.POINTER(structs[_struct_pointer(model, ctype)[0]])      # T * / const T * of a struct -> POINTER(mirror of T)
    if ctype == "char *":
        return C.c_char_p                                       # char * (a caller's text buffer) -> c_char_p
    m = re.fullmatch(r"(?:const )?(\w+) \*", ctype)
    if m and m.group(1) in SCALARS:
        return C.POINTER(SCALARS[m.group(1)])                   # int32_t *, const uint64_t *, ... -> POINTER(c_int32), ...
    raise KeyError(ctype)


def python_structs(lib):
    """{C struct: its ctypes mirror in `lib`} for the structs `lib` has."""
    return {s: getattr(lib, camel(s)) for s in header_model()["structs"] if hasattr(lib, camel(s))}


def _tname(t):
    return getattr(t, "__name__", repr(t))


def check_ctypes_signatures(model, signatures, structs):
    out = ["%s: in the header, not in SIGNATURES" % n for n in sorted(set(model["functions"]) - set(signatures))]
    out += ["%s: in SIGNATURES, not in the header" % n for n in sorted(set(signatures) - set(model["functions"]))]
    for name, f in model["functions"].items():
        if name not in signatures:
            continue
        restype, argtypes = signatures[name]
        try:
            want = [ctypes_image(model, structs, f["returns"], returned=True)] + [ctypes_image(model, structs, t, e) for t, _, e in f["params"]]
        except KeyError as e:
            out.append("%s: no ctypes row for the C type %s" % (name, e))
            continue
        labels = ["the return type"] + ["argument %d (%s %s)" % (i, t, n) for i, (t, n, _) in enumerate(f["params"])]
        if len(argtypes) != len(f["params"]):
            out.append("%s: %d argtypes for %d parameters" % (name, len(argtypes), len(f["params"])))
        out += ["%s: %s is %s, the header's type maps to %s" % (name, label, _tname(have), _tname(exp))
                for label, have, exp in zip(labels, [restype] + list(argtypes), want) if have is not exp]
    return out


# ---- struct layouts: the compiler's, not a second implementation of C's rules ---------------------------------------------------

@functools.lru_cache(maxsize=None)
def compiler_layout(text=None):
    """{struct: {"sizeof": n, field: (offset, size)}} as gcc lays out the structs of a header (default: the header itself)."""
    text = header_text() if text is None else text
    model = parse_header(text)
    lines = ['#include <stdio.h>', '#include "meao.h"', "int main(void) {"]
    for s, fields in model["structs"].items():
        lines.append('  printf("%s sizeof %%zu 0\\n", sizeof(%s));' % (s, s))
        lines += ['  printf("%s %s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));' % (s, n, s, n, s, n) for _, n, _ in fields]
    lines.append("  return 0; }")
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "meao.h"), "w") as f:
            f.write(text)
        with open(os.path.join(tmp, "layout.c"), "w") as f:
            f.write("\n".join(lines) + "\n")
        subprocess.run(["gcc", "-std=c11", "-I" + tmp, os.path.join(tmp, "layout.c"), "-o", os.path.join(tmp, "layout")], check=True)
        printed = subprocess.run([os.path.join(tmp, "layout")], capture_output=True, text=True, check=True).stdout
    layout = {}
    for s, n, a, b in (line.split() for line in printed.splitlines()):
        layout.setdefault(s, {})[n] = int(a) if n == "sizeof" else (int(a), int(b))
    return layout


def check_ctypes_structs(model, structs, layout):
    out = []
    for s, fields in model["structs"].items():
        if s not in structs:
            out.append("%s: no ctypes mirror %s" % (s, camel(s)))
            continue
        mirror, names = structs[s], [n for _, n, _ in fields]
        if [f[0] for f in mirror._fields_] != names:
            out.append("%s: fields %s, the header has %s" % (s, [f[0] for f in mirror._fields_], names))
            continue
        if C.sizeof(mirror) != layout[s]["sizeof"]:
            out.append("%s: sizeof is %d, the compiler's %d" % (s, C.sizeof(mirror), layout[s]["sizeof"]))
        for (ctype, n, extent), (_, have) in zip(fields, mirror._fields_):
            at = (getattr(mirror, n).offset, getattr(mirror, n).size)
            if at != layout[s][n]:
                out.append("%s.%s: (offset, size) is %s, the compiler's %s" % (s, n, at, layout[s][n]))
            want = SCALARS.get(ctype) and (SCALARS[ctype] * extent if extent else SCALARS[ctype])
            if have is not want:
                out.append("%s.%s: %s, the header's %s maps to %s" % (s, n, _tname(have), ctype, _tname(want)))
    return out


# ---- enums and constants in Python ----------------------------------------------------------------------------------------------

def _pass_name(member):
    """MEAO_PASS_UPSAMPLE_3 -> 'upsample_L4_to_L3', MEAO_PASS_RENDER_HQ -> 'render_hq': the entries of _lib.PASS_NAMES."""
    name = member[len("MEAO_PASS_"):].lower()
    m = re.fullmatch(r"upsample_(\d)", name)
    return "upsample_L%d_to_L%d" % (int(m.group(1)) + 1, int(m.group(1))) if m else name


def check_python_constants(model, lib):
    """Every #define and every enum member under its name without MEAO_.  meao_pass is the one exemption: Python carries it as
    the ordered PASS_NAMES, whose order is the enum's."""
    out, named = [], dict(model["defines"])
    for enum, members in model["enums"].items():
        if enum == "meao_pass":
            want = [_pass_name(m) for m, _ in sorted(members.items(), key=lambda kv: kv[1])]
            if list(getattr(lib, "PASS_NAMES", ())) != want or sorted(members.values()) != list(range(len(members))):
                out.append("meao_pass: PASS_NAMES is %s, the header's order gives %s" % (list(getattr(lib, "PASS_NAMES", ())), want))
        else:
            named.update(members)
    return out + ["%s: _lib.%s is %r, the header's value %d" % (name, name[len("MEAO_"):], getattr(lib, name[len("MEAO_"):], None), value)
                  for name, value in named.items() if getattr(lib, name[len("MEAO_"):], None) != value]


# ---- C#: MeaoNative.cs ----------------------------------------------------------------------------------------------------------

def parse_csharp(text):
    """{"lib": the Lib constant, "consts": {name: int}, "enums": {enum: {member: int}}, "structs": {struct: {"layout": kind or
    None, "fields": [[type, name, SizeConst or None]]}}, "imports": {name: {"returns": type, "params": [[marshalling, name]]}}}."""
    text = re.sub(r"//[^\n]*", "", text)
    lib = re.search(r'const string Lib = "(\w+)"', text)
    enums = {}
    for m in re.finditer(r"public enum (\w+)\s*\{(.*?)\}", text, re.S):
        members, value = {}, -1
        for item in filter(None, (i.strip() for i in m.group(2).split(","))):
            name, _, expr = (p.strip() for p in item.partition("="))
            value = int(expr, 0) if expr else value + 1
            members[name] = value
        enums[m.group(1)] = members
    structs = {}
    for m in re.finditer(r"(?:\[StructLayout\(LayoutKind\.(\w+)\)\]\s*)?public struct (\w+)\s*\{(.*?)\}", text, re.S):
        fields = re.findall(r"(?:\[MarshalAs\(UnmanagedType\.ByValArray, SizeConst = (\d+)\)\]\s*)?public ([\w\[\]]+) (\w+);", m.group(3))
        structs[m.group(2)] = {"layout": m.group(1), "fields": [[t, n, int(size) if size else None] for size, t, n in fields]}
    imports = {}
    for m in re.finditer(r"\[DllImport\(Lib\)\]\s*public static extern (\w+) (meao_\w+)\((.*?)\);", text):
        params = [p.strip().rpartition(" ") for p in m.group(3).split(",") if p.strip()]
        imports[m.group(2)] = {"returns": m.group(1), "params": [[how, name.lstrip("@")] for how, _, name in params]}   # @out: the name `out`
    return {"lib": lib and lib.group(1), "consts": {n: int(v) for n, v in re.findall(r"public const int (\w+) = (-?\d+);", text)},
            "enums": enums, "structs": structs, "imports": imports}


CS_SCALARS = {"int32_t": "int", "uint32_t": "uint", "uint64_t": "ulong", "float": "float"}
# C cannot say whether a pointer to a const struct is one object or an array of them: the marshallings each struct is passed by
CS_CONST_STRUCT = {"meao_params": {"ref MeaoParams", "[In] MeaoParams[]"}, "meao_config": {"ref MeaoConfig"},
                   "meao_extent": {"[In] MeaoExtent[]"}, "meao_target_extent": {"[In] MeaoTargetExtent[]"}}


def csharp_images(model, ctype, extent=None, returned=False):
    """The marshallings a [DllImport] may use for a C parameter (or return) type; KeyError for a type without a row."""
    if returned and ctype == "void":
        return {"void"}                                         # return void
    if returned and ctype == "const char *":
        return {"IntPtr"}                                       # a static string: Marshal.PtrToStringAnsi, never freed
    if extent is not None:
        return {"[Out] %s[]" % CS_SCALARS[ctype]}               # float x[N] / uint64_t x[N]: a caller's array the call fills
    if ctype in CS_SCALARS:
        return {CS_SCALARS[ctype]}                              # int32_t -> int, uint64_t -> ulong
    if ctype in OPAQUE:
        return {"IntPtr"}                                       # opaque handles, void *, const void *, meao_stream
    if ctype in HANDLE_OUT and not returned:
        return {"out IntPtr"}                                   # meao_ctx ** / meao_pool **: the created handle
    if ctype in POINTER_ARRAYS:
        return {"IntPtr[]"}                                     # one device or host pointer per frame
    if _struct_pointer(model, ctype):
        struct, const = _struct_pointer(model, ctype)
        if const and struct not in CS_CONST_STRUCT:
            raise KeyError(ctype)
        return CS_CONST_STRUCT[struct] if const else {"out Meao" + camel(struct)}      # non-const struct pointer: filled by the call
    rows = {"int32_t *": {"out int"}, "const int32_t *": {"int[]"},                    # one result; an array of ordinals
            "uint64_t *": {"out ulong"}, "const uint64_t *": {"[In] ulong[]"},           # one result; one pitch per frame
            "char *": {"System.Text.StringBuilder"}}                                   # a caller's text buffer
    return rows[ctype]


def _csharp_name_fits(cname, extent, how, name):
    """A C# parameter carries the header's name, except: `params` is a C# keyword (prm); a header name `out` or `out_<x>` may take
    any name on an `out` / `[Out]` parameter; the fixed-extent arrays bytes / ms carry their extent (bytes7, ms7)."""
    return (name == cname or (cname == "params" and name == "prm")
            or ((cname == "out" or cname.startswith("out_")) and how.startswith(("out ", "[Out] ")))
            or (extent is not None and cname in ("bytes", "ms") and name == "%s%d" % (cname, extent)))


def check_csharp_imports(model, cs):
    out = [] if cs["lib"] == "meao_hip" else ['const string Lib = "meao_hip" is missing (found %r)' % cs["lib"]]
    out += ["%s: in the header, not a [DllImport]" % n for n in sorted(set(model["functions"]) - set(cs["imports"]))]
    out += ["%s: a [DllImport], not in the header" % n for n in sorted(set(cs["imports"]) - set(model["functions"]))]
    for name, f in model["functions"].items():
        if name not in cs["imports"]:
            continue
        imp = cs["imports"][name]
        try:
            returns = csharp_images(model, f["returns"], returned=True)
            allowed = [csharp_images(model, t, e) for t, _, e in f["params"]]
        except KeyError as e:
            out.append("%s: no C# row for the C type %s" % (name, e))
            continue
        if imp["returns"] not in returns:
            out.append("%s: returns %s, the header's %s allows %s" % (name, imp["returns"], f["returns"], sorted(returns)))
        if len(imp["params"]) != len(f["params"]):
            out.append("%s: %d parameters, the header has %d" % (name, len(imp["params"]), len(f["params"])))
            continue
        for (ctype, cname, extent), ok, (how, csname) in zip(f["params"], allowed, imp["params"]):
            if how not in ok:
                out.append("%s: %s %s is marshalled as %s, allowed: %s" % (name, ctype, cname, how, sorted(ok)))
            if not _csharp_name_fits(cname, extent, how, csname):
                out.append("%s: parameter %s is named %s" % (name, cname, csname))
    return out


def check_csharp_structs(model, cs):
    out = []
    for s, fields in model["structs"].items():
        mirror = cs["structs"].get("Meao" + camel(s))
        if mirror is None:
            out.append("%s: no C# struct Meao%s" % (s, camel(s)))
            continue
        if mirror["layout"] != "Sequential":
            out.append("%s: Meao%s is not [StructLayout(LayoutKind.Sequential)]" % (s, camel(s)))
        if [n for _, n, _ in mirror["fields"]] != [n for _, n, _ in fields]:
            out.append("%s: fields %s, the header has %s" % (s, [n for _, n, _ in mirror["fields"]], [n for _, n, _ in fields]))
            continue
        for (ctype, n, extent), (have, _, size) in zip(fields, mirror["fields"]):
            want = (CS_SCALARS[ctype] + "[]", extent) if extent else (CS_SCALARS[ctype], None)        # x[N]: ByValArray, SizeConst = N
            if (have, size) != want:
                out.append("%s.%s: C# has %s (SizeConst %s), the header's %s%s maps to %s (SizeConst %s)"
                           % (s, n, have, size, ctype, "[%d]" % extent if extent else "", want[0], want[1]))
    return out


def check_csharp_enums_and_constants(model, cs, unmirrored=()):
    """Every header enum has its C# enum (MeaoColorFormat <-> meao_color_format) with the same member set and values, or is named
    in `unmirrored` (never both, and nothing the header lacks); the const ints against the #defines, both ways.  meao_status drops
    its ERR_ in C# (MeaoStatus.InvalidArgument)."""
    by_name = {fold(e): e for e in model["enums"]}
    mirrored = {by_name[fold(e)] for e in cs["enums"] if fold(e) in by_name}
    out = ["%s: no C# enum Meao%s, and not listed as deliberately unmirrored" % (e, camel(e))
           for e in model["enums"] if e not in mirrored and e not in unmirrored]
    out += ["%s: listed as unmirrored, but C# has Meao%s" % (e, camel(e)) for e in unmirrored if e in mirrored]
    out += ["%s: listed as unmirrored, but the header does not declare it" % e for e in unmirrored if e not in model["enums"]]
    for enum, members in cs["enums"].items():
        if fold(enum) not in by_name:
            out.append("%s: mirrors no enum of the header" % enum)
            continue
        cmembers = model["enums"][by_name[fold(enum)]]
        prefix = _enum_prefix(cmembers)
        key = {m: fold(re.sub(r"^ERR_", "", m[len(prefix):]) if enum == "MeaoStatus" else m[len(prefix):]) for m in cmembers}
        want = {key[m]: v for m, v in cmembers.items()}
        have = {fold(m): v for m, v in members.items()}
        written = dict({key[m]: m for m in cmembers}, **{fold(m): m for m in members})      # as C# writes it, else as C does
        out += ["%s: member %s is %s, the header's %s has %s" % (enum, written.get(k, k), have.get(k), by_name[fold(enum)], want.get(k))
                for k in sorted(set(have) | set(want)) if have.get(k) != want.get(k)]
    want = {fold(d[len("MEAO_"):]): v for d, v in model["defines"].items()}
    have = {fold(c): v for c, v in cs["consts"].items()}
    names = {fold(c): c for c in cs["consts"]}
    out += ["const int %s is %s, the header's #define has %s" % (names.get(k, k), have.get(k), want.get(k))
            for k in sorted(set(have) | set(want)) if have.get(k) != want.get(k)]
    return out


# ---- C++: the wrapper -----------------------------------------------------------------------------------------------------------

def check_hpp(model, hpp, unwrapped):
    """Every function of the header is called by the wrapper or named in `unwrapped` (why it is not), never both or neither."""
    called = set(re.findall(r"\b(meao_\w+)\s*\(", _strip_comments(hpp)))
    out = ["%s: neither called in the C++ wrapper nor listed as deliberately unwrapped" % n
           for n in model["functions"] if n not in called and n not in unwrapped]
    out += ["%s: listed as unwrapped, but the C++ wrapper calls it" % n for n in unwrapped if n in called]
    out += ["%s: listed as unwrapped, but the header does not declare it" % n for n in unwrapped if n not in model["functions"]]
    return out


# ---- the library ----------------------------------------------------------------------------------------------------------------

def check_exports(model, nm_output):
    """`nm -D --defined-only` of the product library: every function exported, no test hook, no oracle code."""
    exported = set(re.findall(r" T (meao_\w+)", nm_output))
    out = ["%s: declared in the header, not exported" % n for n in model["functions"] if n not in exported]
    out += ["%s: exported by the product library" % n for n in sorted(exported) if n.startswith(("meao_test_", "meao_oracle"))]
    return out


if __name__ == "__main__":
    if sys.argv[1:] != ["--write-snapshot"]:
        sys.exit("usage: python -m tests.abi_model --write-snapshot")
    with open(SNAPSHOT_PATH, "w") as f:
        f.write(dump(header_model()))
    print("wrote %s: %d functions, %d structs, %d enums, %d defines" % ((os.path.relpath(SNAPSHOT_PATH, ROOT),) + tuple(
        len(header_model()[k]) for k in ("functions", "structs", "enums", "defines"))))
