"""The host build of matrix0_amd/csrc/rowpack_core.h with the kernels' lane split as loops (tests/rowpack_shim/rowpack_shim.cpp,
compiled by g++ into tests/_build/librowpack_shim.so), which tests/test_rowpack.py compares with the straight loops of
m0_rowpack_pack_host / m0_rowpack_unpack_host.  load() makes the library and types its functions; pack_lanes() and unpack_lanes()
call it as matrix0_amd.rowpack calls the engine."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

from matrix0_amd import rowpack as rp
from matrix0_amd._abi import RowpackArrays

HERE = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(maxsize=None)
def load():
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "rowpack_shim"), "../_build/librowpack_shim.so"])
    lib = C.CDLL(os.path.join(HERE, "_build", "librowpack_shim.so"))
    lib.rs_pack_lanes.restype = C.c_int
    lib.rs_pack_lanes.argtypes = [C.c_void_p] * 4 + [C.c_int, C.POINTER(RowpackArrays), C.c_void_p]
    lib.rs_unpack_lanes.restype = C.c_int
    lib.rs_unpack_lanes.argtypes = [C.POINTER(RowpackArrays)] + [C.c_void_p] * 4
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def pack_lanes(s, pi, z, mask=None):
    """rowpack.pack_rows through the lane-split loops: a PackedRows"""
    s, pi, z = (np.ascontiguousarray(a, np.float32) for a in (s, pi, z))
    mask = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    n, sizes = len(s), np.zeros(3, np.int64)
    out = None
    for caps in ((0, 0, 0), None):
        npi, nmk, raw = caps if caps is not None else (int(x) for x in sizes)
        out = rp.PackedRows(np.zeros((n, rp.POS_BYTES), np.uint8), np.empty(n, np.float32), np.empty(n + 1, np.int64),
                            np.empty(npi, np.uint16), np.empty(npi, np.float32), np.empty(n + 1, np.int64), np.empty(nmk, np.uint16),
                            np.empty((raw, 19, 8, 8), np.float32), np.empty((raw, 4672), np.float32),
                            None if mask is None else np.empty((raw, 4672), np.uint8))
        a = out.c_arrays()
        rc = load().rs_pack_lanes(_p(s), _p(pi), _p(z), _p(mask), n, C.byref(a), _p(sizes))
        if rc == 0:
            return out
    raise ValueError("rs_pack_lanes refused its own sizes")


def unpack_lanes(packed):
    """rowpack.unpack_rows through the lane-split loops"""
    n = packed.n
    s, pi, z = np.empty((n, 19, 8, 8), np.float32), np.empty((n, 4672), np.float32), np.empty(n, np.float32)
    mask = np.empty((n, 4672), np.uint8) if packed.has_mask else None
    a = packed.c_arrays()
    if load().rs_unpack_lanes(C.byref(a), _p(s), _p(pi), _p(z), _p(mask)) != 0:
        raise ValueError("rs_unpack_lanes refused its arguments")
    return s, pi, z, mask
