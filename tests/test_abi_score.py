"""matrix0_amd/_abi.py against include/m0_score.h (no GPU; the last test needs the built library): the score calls, their options
struct and constants, compared name by name and type by type as tests/test_abi.py compares the main table with m0_engine.h."""
import ctypes as C
import os

from matrix0_amd import _abi, _lib
from tests import test_abi as ta

SCORE_HEADER = os.path.join(os.path.dirname(ta.HEADER), "m0_score.h")


def test_every_score_call_is_in_the_table_with_its_types():
    h = ta.parse_header(SCORE_HEADER)
    assert list(h["functions"]) == list(_abi.SCORE_FUNCTIONS) == ["m0_score_rows", "m0_net_score", "m0_score_bench"]
    assert not set(_abi.SCORE_FUNCTIONS) & (set(_abi.FUNCTIONS) | set(_abi.LIVE_FUNCTIONS))
    for name, (ret, params) in h["functions"].items():
        restype, argtypes = _abi.SCORE_FUNCTIONS[name]
        assert ta.kind_of_ctype(restype) == ret == "i4", name
        assert [ta.kind_of_ctype(a) for a in argtypes] == params, name


def test_the_options_struct_and_the_constants_equal_the_header():
    h = ta.parse_header(SCORE_HEADER)
    assert list(h["structs"]) == list(_abi.SCORE_STRUCTS) == ["m0_score_opts"]
    fields = h["structs"]["m0_score_opts"]
    mirror = _abi.ScoreOpts._fields_
    assert [f for f, _ in fields] == [f for f, _ in mirror] == ["mask_mode", "label_smoothing", "value_loss", "huber_delta"]
    assert [k for _, k in fields] == [ta.kind_of_ctype(t) for _, t in mirror] == ["i4", "f4", "i4", "f4"]
    assert C.sizeof(_abi.ScoreOpts) == 16
    d = h["defines"]
    assert {k[len("M0_SCORE_MASK_"):].lower(): v for k, v in d.items() if k.startswith("M0_SCORE_MASK_")} == _abi.SCORE_MASK
    assert {k[len("M0_SCORE_FLAG_"):].lower(): v for k, v in d.items() if k.startswith("M0_SCORE_FLAG_")} == _abi.SCORE_FLAGS
    assert d["M0_SCORE_COLS"] == _abi.SCORE_COLS == len(_abi.SCORE_COLUMNS) == 8
    assert len(d) == 3 + 3 + 1


def test_the_main_header_includes_the_score_header():
    assert '#include "m0_score.h"' in open(ta.HEADER).read()


def test_the_built_library_exports_the_score_calls():
    L = _lib.lib()
    for name, (restype, argtypes) in _abi.SCORE_FUNCTIONS.items():
        fn = getattr(L, name)
        assert fn.restype is restype and fn.argtypes == argtypes, name
