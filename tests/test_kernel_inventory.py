"""The shape of the library's kernel inventory (tests/kernel_inventory.py), read from its device code without a GPU.

Every render and upsample family is compiled for exactly the six (AOFMT, RTNE, DIV) columns a context can select, and every
downsample family for its eight <VEC, DIV, ROWS> forms: what tests/test_kernel_coverage_gpu.py launches column by column."""
import collections
import itertools

from miniengineao_amd import _lib as L
from tests import kernel_inventory as K


def test_inventory_reads_the_loaded_library():
    names = K.instantiations()
    assert names == K.instantiations(L.LIB_PATH)
    assert len(names) == len(set(names)) == len(K.mangled_names()) and len(names) > 100
    assert "render_kernel<0, false, 0, false>" in names and "downsample_kernel<true, 0, 2>" in names, names[:20]
    assert all("meao::" not in n and "(" not in n for n in names), names[:5]


def test_normalise_takes_mangled_and_demangled_trace_names():
    mangled = K.mangled_names()
    demangled = K.demangle(mangled)
    assert K.normalise(list(mangled)) == K.normalise(demangled) == [K._short()(n) for n in demangled]
    assert K.normalise([mangled[0] + ".kd", "__amd_rocclr_fillBufferAligned"]) == [K._short()(demangled[0])]
    assert set(K.normalise(mangled)) == set(K.instantiations())


def test_render_and_upsample_families_cover_exactly_the_six_columns():
    families = collections.defaultdict(set)
    for n in K.instantiations():
        col = K.column_of(n)
        if col is None or col[0] == "ds":
            continue
        base, args = K.split(n)
        families[(base, tuple(args[3:]))].add(col)
    assert len(families) >= 40, sorted(families)
    for fam, cols in sorted(families.items()):
        assert cols == set(K.COLUMNS), (fam, sorted(cols))
    assert not [n for n in K.instantiations() if K.column_of(n) and K.column_of(n)[1:] == ("true", "0")]


def test_every_downsample_family_has_its_eight_forms():
    forms = collections.defaultdict(set)
    for n in K.instantiations():
        base, args = K.split(n)
        if base.startswith("downsample"):
            forms[base].add(tuple(args))
    want = set(itertools.product(("false", "true"), ("0", "1"), ("1", "2")))
    assert {"downsample_kernel", "downsample_frames_kernel", "downsample_pitched_kernel", "downsample_pitched_frames_kernel",
            "downsample_linear_kernel", "downsample_linear_frames_kernel"} <= set(forms), sorted(forms)
    for base, got in sorted(forms.items()):
        assert got == want, (base, sorted(got))
