"""matrix0_amd/_abi.py against include/m0_gumbel.h (no GPU; the last test needs the built library): the Gumbel root search's calls
and its options struct, compared name by name and type by type as tests/test_abi.py compares the main table with m0_engine.h."""
import ctypes as C
import os

from matrix0_amd import _abi, _lib
from tests import test_abi as ta

GUMBEL_HEADER = os.path.join(os.path.dirname(ta.HEADER), "m0_gumbel.h")


def test_every_gumbel_call_is_in_the_table_with_its_types():
    h = ta.parse_header(GUMBEL_HEADER)
    assert list(h["functions"]) == list(_abi.GUMBEL_FUNCTIONS) == ["m0_selfplay_set_gumbel", "m0_search_gumbel_result",
                                                                   "m0_gumbel_schedule", "m0_gumbel_improve"]
    assert not set(_abi.GUMBEL_FUNCTIONS) & (set(_abi.FUNCTIONS) | set(_abi.LIVE_FUNCTIONS) | set(_abi.SCORE_FUNCTIONS))
    for name, (ret, params) in h["functions"].items():
        restype, argtypes = _abi.GUMBEL_FUNCTIONS[name]
        assert ta.kind_of_ctype(restype) == ret == "i4", name
        assert [ta.kind_of_ctype(a) for a in argtypes] == params, name


def test_the_options_struct_equals_the_header():
    h = ta.parse_header(GUMBEL_HEADER)
    assert list(h["structs"]) == list(_abi.GUMBEL_STRUCTS) == ["m0_gumbel_cfg"]
    fields = h["structs"]["m0_gumbel_cfg"]
    mirror = _abi.GumbelCfg._fields_
    assert [f for f, _ in fields] == [f for f, _ in mirror] == ["max_considered", "c_visit", "c_scale"]
    assert [k for _, k in fields] == [ta.kind_of_ctype(t) for _, t in mirror] == ["i4", "f8", "f8"]
    assert C.sizeof(_abi.GumbelCfg) == 24
    assert not h["defines"]


def test_the_main_header_includes_the_gumbel_header_and_keeps_its_own_structs():
    assert '#include "m0_gumbel.h"' in open(ta.HEADER).read()
    main = ta.parse_header()
    assert "m0_gumbel_cfg" not in main["structs"] and not set(_abi.GUMBEL_FUNCTIONS) & set(main["functions"])


def test_the_built_library_exports_the_gumbel_calls():
    L = _lib.lib()
    for name, (restype, argtypes) in _abi.GUMBEL_FUNCTIONS.items():
        fn = getattr(L, name)
        assert fn.restype is restype and fn.argtypes == argtypes, name
