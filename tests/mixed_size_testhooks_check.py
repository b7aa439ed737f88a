"""Body of tests/test_mixed_size_gpu.py::test_mixed_calls_neither_allocate_nor_synchronise.  Runs in its own process against the
`testhooks` variant library (MEAO_LIB_PATH; -DMEAO_TESTING=1), the only build that exports meao_test_counters (out[0] = arena
allocations attempted, out[1] = synchronising HIP calls of the context, both since meao_create) and the fault injection
meao_test_fail_next_allocs.  Ten mixed DEVICE calls -- more than the ring of 8 tables holds, so slots are reused -- with every
allocation of intermediates set to fail: both counters stay where they were and every frame is exact.  Exit code 0 = passed."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from miniengineao_amd import _lib as L
from oracle import oracle
from tests import mixed_size as M


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
    base = M.base_settings(oracle)
    ao = M.context(base, pipelined=True)
    try:
        lists = [M.ORDER, M.EDGES, M.ORDER[::-1], M.ALIGNED, M.ORDER + M.EDGES[:4]]
        # every frame on the device before the calls start; a warm-up call first, so that whatever a context sets up once
        # (the profiler is off, nothing is staged) is behind it
        calls = [M.MixedCall(torch, oracle, base, lists[k % len(lists)], per_frame=bool(k % 2), pitched=(k % 3 == 2)) for k in range(10)]
        warm = M.MixedCall(torch, oracle, base, M.ORDER)
        warm.execute(ao)
        torch.cuda.synchronize()
        allocs, syncs = counters(lib, ao)
        assert allocs == 1                                  # meao_create
        assert inject(ao._ctx, 1000) == L.OK                # any allocation of intermediates from here on would fail
        for k, call in enumerate(calls):
            call.execute(ao)                                # every call returns MEAO_OK (L.check raises otherwise)
            if k % 4 == 3:
                torch.cuda.synchronize()                    # the host stays fewer than 8 per-frame calls ahead: the ring's back-pressure
                                                            # (a counted wait, include/meao.h) is not what this check is about
        assert counters(lib, ao) == (allocs, syncs), (counters(lib, ao), allocs, syncs)
        torch.cuda.synchronize()
        for k, call in enumerate(calls):
            call.check(ao, debug_buffers=False, what="call %d" % k)
        assert inject(ao._ctx, 0) == L.OK
    finally:
        ao.close()
    print("mixed size testhooks check ok")


if __name__ == "__main__":
    main()
