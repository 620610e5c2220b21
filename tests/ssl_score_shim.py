"""The host build of matrix0_amd/csrc/ssl_score_core.h and ssl_targets_core.h that the SSL score tests compare with the float64
reference and with the kernel: tests/ssl_score_shim/ssl_score_shim.cpp, compiled by g++ into tests/_build/libssl_score_shim.so.
load() makes the library and types its functions; score_rows() and targets_planes() call them as m0_ssl_score_rows and
m0_ssl_targets_planes are called."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

from matrix0_amd import _abi

HERE = os.path.dirname(os.path.abspath(__file__))
SENTINEL = -7.0


@functools.lru_cache(maxsize=None)
def load():
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "ssl_score_shim"), "../_build/libssl_score_shim.so"])
    lib = C.CDLL(os.path.join(HERE, "_build", "libssl_score_shim.so"))
    lib.sss_score_rows.restype = C.c_int
    lib.sss_score_rows.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.sss_targets_planes.restype = C.c_int
    lib.sss_targets_planes.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.sss_math.restype = None
    lib.sss_math.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float32)


def score_rows(heads, tasks, planes, targets=None):
    """f32 [B, 16]; tasks: the bitmask; ValueError for the arguments the core refuses."""
    heads, planes, targets = _f(heads), _f(planes), _f(targets)
    rows = np.full((len(planes), _abi.SSL_SCORE_COLS), SENTINEL, np.float32)
    if load().sss_score_rows(_p(heads), int(tasks), _p(planes), _p(targets), len(planes), _p(rows)) != 0:
        raise ValueError("sss_score_rows refused its arguments")
    return rows


def targets_planes(planes, fill=SENTINEL):
    """(out f32 [n,17,64] prefilled with `fill`, status i32 [n])"""
    planes = _f(planes)
    out = np.full((len(planes), 17, 64), fill, np.float32)
    status = np.full(len(planes), -1, np.int32)
    assert load().sss_targets_planes(_p(planes), len(planes), _p(out), _p(status)) == 0
    return out, status


def math(x, which):
    """the core's exp_le0 / log_ge1 / log1p_series ("exp", "log", "log1p") of every element"""
    x = _f(x).reshape(-1)
    y = np.empty_like(x)
    load().sss_math(_p(x), len(x), ("exp", "log", "log1p").index(which), _p(y))
    return y
