"""matrix0_amd/_abi.py against include/m0_batch.h (no GPU; the last tests need the built library): the calls of the resident row
store, compared name by name and type by type as tests/test_abi.py compares the main table with m0_engine.h."""
import ctypes as C
import os

import numpy as np

from matrix0_amd import _abi, _lib
from tests import test_abi as ta

BATCH_HEADER = os.path.join(os.path.dirname(ta.HEADER), "m0_batch.h")
NAMES = ["m0_rowstore_create", "m0_rowstore_destroy", "m0_rowstore_append", "m0_rowstore_evict", "m0_rowstore_info",
         "m0_rowstore_batch", "m0_rowstore_batch_host", "m0_rowstore_bench"]


def test_every_batch_call_is_in_the_table_with_its_types():
    h = ta.parse_header(BATCH_HEADER)
    assert list(h["functions"]) == list(_abi.BATCH_FUNCTIONS) == NAMES
    others = (set(_abi.FUNCTIONS) | set(_abi.LIVE_FUNCTIONS) | set(_abi.SCORE_FUNCTIONS) | set(_abi.SSL_SCORE_FUNCTIONS) |
              set(_abi.GUMBEL_FUNCTIONS) | set(_abi.AUGMENT_FUNCTIONS) | set(_abi.PROOF_FUNCTIONS) | set(_abi.ROWPACK_FUNCTIONS))
    assert not set(_abi.BATCH_FUNCTIONS) & others
    for name, (ret, params) in h["functions"].items():
        restype, argtypes = _abi.BATCH_FUNCTIONS[name]
        assert ta.kind_of_ctype(restype) == ret, name
        assert [ta.kind_of_ctype(a) for a in argtypes] == params, name
    assert not h["structs"]                                            # the handle is opaque
    assert h["defines"] == {"M0_ROWSTORE_HOST": _abi.ROWSTORE_HOST, "M0_ROWSTORE_INFO": len(_abi.ROWSTORE_INFO)}


def test_the_main_header_includes_the_batch_header_behind_the_rowpack_header():
    text = open(ta.HEADER).read()
    assert 0 < text.index('#include "m0_rowpack.h"') < text.index('#include "m0_batch.h"')
    main = ta.parse_header()
    assert not set(_abi.BATCH_FUNCTIONS) & set(main["functions"])
    assert not {"m0_rowstore"} & set(main["structs"])


def test_the_built_library_exports_the_batch_calls():
    L = _lib.lib()
    for name, (restype, argtypes) in _abi.BATCH_FUNCTIONS.items():
        fn = getattr(L, name)
        assert fn.restype is restype and fn.argtypes == argtypes, name


def test_null_handles_and_null_arguments_are_refused_with_a_message():
    L = _lib.lib()
    out = np.zeros(6, np.int64)
    first = C.c_int64(0)
    a = _abi.RowpackArrays()
    rows = np.zeros(1, np.int64)
    s, pi, z = np.zeros(19 * 64, np.float32), np.zeros(4672, np.float32), np.zeros(1, np.float32)
    calls = [lambda: L.m0_rowstore_append(None, C.byref(a), C.byref(first)),
             lambda: L.m0_rowstore_evict(None, 0),
             lambda: L.m0_rowstore_info(None, _lib.ptr(out)),
             lambda: L.m0_rowstore_batch(None, _lib.ptr(rows), None, 1, _lib.ptr(s), _lib.ptr(pi), _lib.ptr(z), None, 0, None),
             lambda: L.m0_rowstore_batch_host(None, _lib.ptr(rows), None, 1, _lib.ptr(s), _lib.ptr(pi), _lib.ptr(z), None),
             lambda: L.m0_rowstore_batch_host(C.byref(a), _lib.ptr(rows), None, 1, _lib.ptr(s), _lib.ptr(pi), _lib.ptr(z), None),
             lambda: L.m0_rowstore_bench(0, 0, 1, None, None, None)]
    for k, call in enumerate(calls):
        assert call() == _lib.M0_ERR_INVALID and _lib.last_error(), k
    L.m0_rowstore_destroy(None)                                        # nothing to do
    assert not L.m0_rowstore_create(-2, 1) and _lib.last_error()
    h = L.m0_rowstore_create(_abi.ROWSTORE_HOST, 1)
    try:
        assert L.m0_rowstore_append(h, None, C.byref(first)) == _lib.M0_ERR_INVALID and "null" in _lib.last_error()
        assert L.m0_rowstore_append(h, C.byref(a), None) == _lib.M0_ERR_INVALID
        assert L.m0_rowstore_info(h, None) == _lib.M0_ERR_INVALID
        assert L.m0_rowstore_info(h, _lib.ptr(out)) == _lib.M0_OK and out.tolist() == [0, 0, 0, 0, 0, 0]
    finally:
        L.m0_rowstore_destroy(h)
