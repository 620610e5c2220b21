"""matrix0_amd/_abi.py against include/m0_rowpack.h (no GPU; one test needs the built library): the packed-row calls, constants
and structs, compared name by name and type by type as tests/test_abi.py compares the main table with m0_engine.h."""
import ctypes as C
import os

import numpy as np

from matrix0_amd import _abi, _lib, rowpack
from tests import test_abi as ta

ROWPACK_HEADER = os.path.join(os.path.dirname(ta.HEADER), "m0_rowpack.h")


def _kind(t):
    """ta.kind_of_ctype for the types of this header's structs"""
    return ("array", _kind(t._type_), t._length_) if issubclass(t, C.Array) else ta.kind_of_ctype(t)


def test_every_rowpack_call_is_in_the_table_with_its_types():
    h = ta.parse_header(ROWPACK_HEADER)
    assert list(h["functions"]) == list(_abi.ROWPACK_FUNCTIONS) == ["m0_rowpack_pack", "m0_rowpack_unpack", "m0_rowpack_pack_host",
                                                                    "m0_rowpack_unpack_host", "m0_net_score_packed", "m0_rowpack_bench"]
    others = (set(_abi.FUNCTIONS) | set(_abi.LIVE_FUNCTIONS) | set(_abi.SCORE_FUNCTIONS) | set(_abi.SSL_SCORE_FUNCTIONS) |
              set(_abi.GUMBEL_FUNCTIONS) | set(_abi.AUGMENT_FUNCTIONS) | set(_abi.PROOF_FUNCTIONS))
    assert not set(_abi.ROWPACK_FUNCTIONS) & others
    for name, (ret, params) in h["functions"].items():
        restype, argtypes = _abi.ROWPACK_FUNCTIONS[name]
        assert ta.kind_of_ctype(restype) == ret == "i4", name
        assert [ta.kind_of_ctype(a) for a in argtypes] == params, name


def test_the_kinds_and_the_structs_equal_the_header():
    h = ta.parse_header(ROWPACK_HEADER)
    d = h["defines"]
    assert d.pop("M0_ROWPACK_VERSION") == _abi.ROWPACK_VERSION == 1
    masks = {k[len("M0_ROWPACK_MASK_"):].lower(): v for k, v in d.items() if k.startswith("M0_ROWPACK_MASK_")}
    rows = {k[len("M0_ROWPACK_"):].lower(): v for k, v in d.items() if not k.startswith("M0_ROWPACK_MASK_")}
    assert masks == _abi.ROWPACK_MASK_KINDS == {"none": 0, "legal": 1, "list": 2}
    assert rows == _abi.ROWPACK_ROW_KINDS == {"packed": 0, "raw": 1}
    assert list(h["structs"]) == list(_abi.ROWPACK_STRUCTS) == ["m0_rowpack_pos", "m0_rowpack_arrays"]
    for name, fields in h["structs"].items():
        mirror = _abi.ROWPACK_STRUCTS[name]._fields_
        assert [f for f, _ in fields] == [f for f, _ in mirror], name
        assert [k for _, k in fields] == [_kind(t) for _, t in mirror], name
    # the packed position: at most 104 bytes, twelve bitboards first; numpy's view of it is the same layout
    assert C.sizeof(_abi.RowpackPos) == rowpack.POS_DTYPE.itemsize == 104
    assert [(n, rowpack.POS_DTYPE.fields[n][1]) for n in rowpack.POS_DTYPE.names] == \
        [(n, getattr(_abi.RowpackPos, n).offset) for n, _ in _abi.RowpackPos._fields_]
    assert rowpack.ARRAY_KEYS == tuple(f for f, _ in _abi.RowpackArrays._fields_[4:])
    assert np.dtype(np.int64).itemsize * 4 == _abi.RowpackArrays.pos.offset


def test_the_main_header_includes_the_rowpack_header():
    assert '#include "m0_rowpack.h"' in open(ta.HEADER).read()
    main = ta.parse_header()
    assert not set(_abi.ROWPACK_FUNCTIONS) & set(main["functions"]) and not set(_abi.ROWPACK_STRUCTS) & set(main["structs"])


def test_the_built_library_exports_the_rowpack_calls():
    L = _lib.lib()
    for name, (restype, argtypes) in _abi.ROWPACK_FUNCTIONS.items():
        fn = getattr(L, name)
        assert fn.restype is restype and fn.argtypes == argtypes, name


def test_the_host_calls_refuse_null_arguments_and_say_why():
    L = _lib.lib()
    sizes = np.zeros(3, np.int64)
    a = _abi.RowpackArrays()
    assert L.m0_rowpack_pack_host(None, None, None, None, 1, C.byref(a), _lib.ptr(sizes)) == _lib.M0_ERR_INVALID
    assert L.m0_rowpack_unpack_host(C.byref(a), None, None, None, None) == _lib.M0_ERR_INVALID
    assert _lib.last_error()
