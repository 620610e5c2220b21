"""The host build of matrix0_amd/csrc/augment_core.h that tests/test_augment.py compares with tests/augment_ref.py:
tests/augment_shim/augment_shim.cpp, compiled by g++ into tests/_build/libaugment_shim.so.  load() makes the library and types its
functions; augment_rows() calls it as m0_augment_rows is called, tables() hands out the core's constexpr tables."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(maxsize=None)
def load():
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "augment_shim"), "../_build/libaugment_shim.so"])
    lib = C.CDLL(os.path.join(HERE, "_build", "libaugment_shim.so"))
    lib.as_augment_rows.restype = C.c_int
    lib.as_augment_rows.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 3
    lib.as_tables.restype = C.c_int
    lib.as_tables.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    lib.as_source_column.restype = C.c_int
    lib.as_source_column.argtypes = [C.c_int, C.c_int]
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def augment_rows(s, pi, mask, kinds):
    """(s', pi', mask' or None) of f32 [B,P,8,8], f32 [B,4672], u8 [B,4672] or None and u8 [B]; ValueError for what the core refuses"""
    s, pi = np.ascontiguousarray(s, dtype=np.float32), np.ascontiguousarray(pi, dtype=np.float32)
    mask = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    kinds = np.ascontiguousarray(kinds, dtype=np.uint8)
    s_out, pi_out = np.empty_like(s), np.empty_like(pi)
    m_out = None if mask is None else np.empty_like(mask)
    if load().as_augment_rows(_p(s), s.shape[1], _p(pi), _p(mask), _p(kinds), len(s), _p(s_out), _p(pi_out), _p(m_out)) != 0:
        raise ValueError("as_augment_rows refused its arguments")
    return s_out, pi_out, m_out


def tables(kind):
    """(perm i32 [73], squares i32 [64]) of the core for a kind 0, 1, 2"""
    perm, squares = np.full(73, -1, np.int32), np.full(64, -1, np.int32)
    if load().as_tables(int(kind), _p(perm), _p(squares)) != 0:
        raise ValueError("no such kind")
    return perm, squares
