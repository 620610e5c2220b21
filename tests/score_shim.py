"""The host build of matrix0_amd/csrc/score_core.h that tests/test_score.py compares with the float64 reference:
tests/score_shim/score_shim.cpp, compiled by g++ into tests/_build/libscore_shim.so.  load() makes the library and types its one
function; score_rows() calls it as M0Backend / m0_score_rows are called."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

from matrix0_amd import _abi

HERE = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(maxsize=None)
def load():
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "score_shim"), "../_build/libscore_shim.so"])
    lib = C.CDLL(os.path.join(HERE, "_build", "libscore_shim.so"))
    lib.ss_score_rows.restype = C.c_int
    lib.ss_score_rows.argtypes = [C.c_void_p] * 5 + [C.c_int, C.POINTER(_abi.ScoreOpts), C.c_void_p]
    return lib


def score_rows(logits, value, pi, z, mask, *, mask_mode, label_smoothing=0.0, value_loss="mse", huber_delta=1.0):
    """f32 [B, 8]; ValueError for the arguments the core refuses."""
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    logits, value, pi, z = f(logits), f(value), f(pi), f(z)
    mask = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    opts = _abi.ScoreOpts(_abi.SCORE_MASK[mask_mode], label_smoothing, {"mse": 0, "huber": 1}[value_loss], huber_delta)
    rows = np.full((logits.shape[0], _abi.SCORE_COLS), -7.0, np.float32)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    if load().ss_score_rows(p(logits), p(value), p(pi), p(z), p(mask), logits.shape[0], C.byref(opts), p(rows)) != 0:
        raise ValueError("ss_score_rows refused its arguments")
    return rows
