"""Body of tests/test_dynamic_resolution_gpu.py::test_resize_inside_a_reservation_neither_allocates_nor_synchronises.  Runs in its own
process against the `testhooks` variant library (MEAO_LIB_PATH; -DMEAO_TESTING=1), the only build that exports meao_test_counters
(out[0] = arena allocations attempted, out[1] = synchronising HIP calls of the context, both since meao_create) and the fault
injection meao_test_fail_next_allocs.  Exit code 0 = passed."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from miniengineao_amd import _lib as L
from oracle import oracle
from tests import dynamic_resolution as D


def counters(lib, ao):
    out = (C.c_uint64 * 2)()
    assert lib.meao_test_counters(ao._ctx, out) == L.OK
    return out[0], out[1]


def main():
    lib = L.load()
    lib.meao_test_counters.restype, lib.meao_test_counters.argtypes = C.c_int32, [C.c_void_p, C.POINTER(C.c_uint64)]   # AttributeError
    inject = lib.meao_test_fail_next_allocs                                                                             # unless testhooks
    inject.restype, inject.argtypes = C.c_int32, [C.c_void_p, C.c_int32]
    oracle.build()
    sizes = [D.A, D.B, D.A, D.C3, D.B, (97, 61), D.RES, D.B, (33, 17), D.A]
    st = D.Stream(torch, oracle, 0, False, sizes[0])
    ao = st.ao
    try:
        ao.set_profiling(False)
        steps = [st.batch(700 + k, w, h) for k, (w, h) in enumerate(sizes)]          # every frame on the device before the stream starts
        tail = st.batch(720, *D.B)
        torch.cuda.synchronize()
        assert ao.capacity == D.RES
        allocs, syncs = counters(lib, ao)
        assert allocs == 2                                  # meao_create and meao_reserve
        assert inject(ao._ctx, 1000) == L.OK                # any allocation of intermediates from here on would fail

        # DEVICE / DEVICE executes on one stream, a resize inside the reservation before each one, sized announcements; every call
        # returns MEAO_OK (L.check raises otherwise)
        for k, b in enumerate(steps):
            ao.resize(*b["size"])
            if k + 1 < len(steps):
                st.announce(steps[k + 1])
            st.execute(b)
        assert counters(lib, ao) == (allocs, syncs), (counters(lib, ao), allocs, syncs)
        torch.cuda.synchronize()
        for b in steps:
            st.check(b)                                     # (meao_synchronize: counted from here on)

        # a reservation that cannot be allocated: out of memory, and the context is as it was -- size, reservation, a ready prefetch
        allocs, syncs = counters(lib, ao)
        st.announce(tail)
        st.execute(steps[-1])
        try:
            ao.reserve(512, 300)
            raise AssertionError("meao_reserve succeeded with the injection armed")
        except L.MeaoError as e:
            assert e.status == L.ERR_OUT_OF_MEMORY, e.status
        assert ao.capacity == D.RES and (ao.width, ao.height) == sizes[-1]
        assert counters(lib, ao)[0] == allocs + 1
        ao.resize(*D.B)
        assert st.downsample_ms(tail) == 0                  # the ready set survived the failed call and the resize; the result is exact
        st.check(steps[-1])

        # outside the reservation a resize allocates once, and the reservation grows
        assert inject(ao._ctx, 0) == L.OK
        allocs = counters(lib, ao)[0]
        ao.resize(500, 100)
        assert counters(lib, ao)[0] == allocs + 1 and ao.capacity == (500, 272)
        ao.resize(100, 300)
        assert counters(lib, ao)[0] == allocs + 2 and ao.capacity == (500, 300)
        ao.resize(*D.A)                                      # inside it again: none
        assert counters(lib, ao)[0] == allocs + 2
        last = st.batch(721, *D.A)
        assert st.downsample_ms(last) > 0
    finally:
        ao.close()
    print("dynamic resolution testhooks check ok")


if __name__ == "__main__":
    main()
