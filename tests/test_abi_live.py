"""matrix0_amd/_abi.py against include/m0_analysis_live.h (no GPU; the last test needs the built library): the live-search calls
of the analysis engine, compared name by name and type by type as tests/test_abi.py compares the main table with m0_engine.h."""
import os

from matrix0_amd import _abi, _lib
from tests import test_abi as ta

LIVE_HEADER = os.path.join(os.path.dirname(ta.HEADER), "m0_analysis_live.h")


def test_every_live_call_is_in_the_table_with_its_types():
    h = ta.parse_header(LIVE_HEADER)
    assert not h["structs"] and not h["defines"]
    assert list(h["functions"]) == list(_abi.LIVE_FUNCTIONS) == [
        "m0_analysis_submit_keep", "m0_analysis_peek", "m0_analysis_stop", "m0_analysis_continue", "m0_analysis_release",
        "m0_analysis_held"]
    assert not set(_abi.LIVE_FUNCTIONS) & set(_abi.FUNCTIONS)
    for name, (ret, params) in h["functions"].items():
        restype, argtypes = _abi.LIVE_FUNCTIONS[name]
        assert ta.kind_of_ctype(restype) == ret == "i4", name
        assert [ta.kind_of_ctype(a) for a in argtypes] == params, name


def test_the_main_header_includes_the_live_header():
    text = open(ta.HEADER).read()
    assert '#include "m0_analysis_live.h"' in text


def test_the_built_library_exports_the_live_calls():
    L = _lib.lib()
    for name, (restype, argtypes) in _abi.LIVE_FUNCTIONS.items():
        fn = getattr(L, name)
        assert fn.restype is restype and fn.argtypes == argtypes, name
