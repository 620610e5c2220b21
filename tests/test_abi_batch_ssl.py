"""matrix0_amd/_abi.py against include/m0_batch_ssl.h (no GPU; the last tests need the built library): the calls that give a batch
the SSL target maps of its rows, compared name by name and type by type as tests/test_abi.py compares the main table with
m0_engine.h.  include/m0_batch.h and its table stay as they were (tests/test_abi_batch.py)."""
import ctypes as C
import os

import numpy as np

from matrix0_amd import _abi, _lib
from tests import test_abi as ta

HEADER = os.path.join(os.path.dirname(ta.HEADER), "m0_batch_ssl.h")
NAMES = ["m0_rowstore_batch_ssl", "m0_rowstore_batch_ssl_host", "m0_rowstore_bench_ssl"]


def test_every_call_is_in_the_table_with_its_types():
    h = ta.parse_header(HEADER)
    assert list(h["functions"]) == list(_abi.BATCH_SSL_FUNCTIONS) == NAMES
    for name, (ret, params) in h["functions"].items():
        restype, argtypes = _abi.BATCH_SSL_FUNCTIONS[name]
        assert ta.kind_of_ctype(restype) == ret == "i4", name
        assert [ta.kind_of_ctype(a) for a in argtypes] == params, name
    assert not h["structs"]
    assert h["defines"] == {"M0_BATCH_SSL_CH": _abi.BATCH_SSL_CH} == {"M0_BATCH_SSL_CH": 17}
    # the new calls are the old ones with two more pointers in front of outputs_on_device (or at the end)
    old, new = _abi.BATCH_FUNCTIONS["m0_rowstore_batch"][1], _abi.BATCH_SSL_FUNCTIONS["m0_rowstore_batch_ssl"][1]
    assert new == old[:8] + [_abi.vp, _abi.vp] + old[8:]
    assert _abi.BATCH_SSL_FUNCTIONS["m0_rowstore_batch_ssl_host"][1] == _abi.BATCH_FUNCTIONS["m0_rowstore_batch_host"][1] + [_abi.vp] * 2
    assert _abi.BATCH_SSL_FUNCTIONS["m0_rowstore_bench_ssl"] == _abi.BATCH_FUNCTIONS["m0_rowstore_bench"]


def test_the_new_names_sit_in_no_other_table_and_in_neither_older_header():
    others = (set(_abi.FUNCTIONS) | set(_abi.LIVE_FUNCTIONS) | set(_abi.SCORE_FUNCTIONS) | set(_abi.SSL_SCORE_FUNCTIONS) |
              set(_abi.GUMBEL_FUNCTIONS) | set(_abi.AUGMENT_FUNCTIONS) | set(_abi.PROOF_FUNCTIONS) | set(_abi.ROWPACK_FUNCTIONS) |
              set(_abi.BATCH_FUNCTIONS) | set(_abi.BUDGET_FUNCTIONS))
    assert not set(NAMES) & others
    text = open(ta.HEADER).read()
    assert 0 < text.index('#include "m0_batch.h"') < text.index('#include "m0_batch_ssl.h"')
    assert not set(NAMES) & set(ta.parse_header()["functions"])
    batch = ta.parse_header(os.path.join(os.path.dirname(ta.HEADER), "m0_batch.h"))
    assert not set(NAMES) & set(batch["functions"]) and "M0_BATCH_SSL_CH" not in batch["defines"]


def test_the_built_library_exports_the_calls():
    L = _lib.lib()
    for name, (restype, argtypes) in _abi.BATCH_SSL_FUNCTIONS.items():
        fn = getattr(L, name)
        assert fn.restype is restype and fn.argtypes == argtypes, name


def test_null_arguments_are_refused_with_a_message():
    L = _lib.lib()
    a = _abi.RowpackArrays()
    rows = np.zeros(1, np.int64)
    s, pi, z = np.zeros(19 * 64, np.float32), np.zeros(4672, np.float32), np.zeros(1, np.float32)
    ssl, status = np.full(17 * 64, -7, np.float32), np.full(1, -7, np.int32)
    p = _lib.ptr
    calls = [lambda: L.m0_rowstore_batch_ssl(None, p(rows), None, 1, p(s), p(pi), p(z), None, p(ssl), p(status), 0, None),
             lambda: L.m0_rowstore_batch_ssl_host(None, p(rows), None, 1, p(s), p(pi), p(z), None, p(ssl), p(status)),
             lambda: L.m0_rowstore_batch_ssl_host(C.byref(a), p(rows), None, 1, p(s), p(pi), p(z), None, p(ssl), p(status)),
             lambda: L.m0_rowstore_bench_ssl(0, 0, 1, None, None, None),
             lambda: L.m0_rowstore_bench_ssl(0, 8, 1, None, None, None)]
    for k, call in enumerate(calls):
        assert call() == _lib.M0_ERR_INVALID and _lib.last_error(), k
    h = L.m0_rowstore_create(_abi.ROWSTORE_HOST, 0)
    try:
        for maps, st in ((None, p(status)), (p(ssl), None)):
            assert L.m0_rowstore_batch_ssl(h, p(rows), None, 1, p(s), p(pi), p(z), None, maps, st, 0, None) == _lib.M0_ERR_INVALID
            assert "null" in _lib.last_error()
        assert L.m0_rowstore_batch_ssl(h, p(rows), None, 1, p(s), p(pi), p(z), None, p(ssl), p(status), 0, None) == _lib.M0_ERR_INVALID
        assert "0" in _lib.last_error()                                    # nothing is resident: the id is named
    finally:
        L.m0_rowstore_destroy(h)
    assert (ssl == -7).all() and (status == -7).all()
