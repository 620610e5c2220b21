"""matrix0_amd/_abi.py against include/m0_ssl_score.h (no GPU; the last test needs the built library): the SSL score calls and
their constants, compared name by name and type by type as tests/test_abi.py compares the main table with m0_engine.h."""
import os

from matrix0_amd import _abi, _lib
from tests import test_abi as ta

SSL_SCORE_HEADER = os.path.join(os.path.dirname(ta.HEADER), "m0_ssl_score.h")


def test_every_ssl_score_call_is_in_the_table_with_its_types():
    h = ta.parse_header(SSL_SCORE_HEADER)
    assert list(h["functions"]) == list(_abi.SSL_SCORE_FUNCTIONS) == ["m0_ssl_score_rows", "m0_net_score_ssl", "m0_ssl_targets_planes",
                                                                      "m0_ssl_score_bench"]
    assert not set(_abi.SSL_SCORE_FUNCTIONS) & (set(_abi.FUNCTIONS) | set(_abi.LIVE_FUNCTIONS) | set(_abi.SCORE_FUNCTIONS) |
                                                set(_abi.GUMBEL_FUNCTIONS))
    for name, (ret, params) in h["functions"].items():
        restype, argtypes = _abi.SSL_SCORE_FUNCTIONS[name]
        assert ta.kind_of_ctype(restype) == ret == "i4", name
        assert [ta.kind_of_ctype(a) for a in argtypes] == params, name
    # the options of m0_net_score_ssl are m0_net_score's
    assert _abi.SSL_SCORE_FUNCTIONS["m0_net_score_ssl"][1][7] is _abi.SCORE_FUNCTIONS["m0_net_score"][1][6]


def test_the_constants_equal_the_header_and_the_header_has_no_struct():
    h = ta.parse_header(SSL_SCORE_HEADER)
    d = h["defines"]
    assert not h["structs"]
    assert {k[len("M0_SSL_SCORE_FLAG_"):].lower(): v for k, v in d.items() if k.startswith("M0_SSL_SCORE_FLAG_")} == _abi.SSL_SCORE_FLAGS
    assert _abi.SSL_SCORE_FLAGS == {"planes": 1, "nonfinite": 2, "mismatch": 4}
    assert d["M0_SSL_SCORE_COLS"] == _abi.SSL_SCORE_COLS == len(_abi.SSL_SCORE_COLUMNS) == 16
    assert len(d) == 1 + 3 and _abi.SSL_SCORE_COLUMNS[-1] == "flags" and len(set(_abi.SSL_SCORE_COLUMNS)) == 16
    # the task order of the head channels and of a row's loss columns is the order of the M0_SSL_* bits
    assert [c[:-len("_loss")] for c in _abi.SSL_SCORE_COLUMNS[:5]] == list(_abi.SSL_BITS) == _lib.SSL_ORDER


def test_the_main_header_includes_the_ssl_score_header_and_keeps_its_own_table():
    text = open(ta.HEADER).read()
    assert '#include "m0_ssl_score.h"' in text and text.index('#include "m0_score.h"') < text.index('#include "m0_ssl_score.h"')
    main = ta.parse_header()
    assert not set(_abi.SSL_SCORE_FUNCTIONS) & set(main["functions"])
    assert not [k for k in main["defines"] if k.startswith("M0_SSL_SCORE_")]
    assert "m0_ssl_score.h" in open(os.path.join(os.path.dirname(ta.HEADER), "m0_score.h")).read()


def test_the_built_library_exports_the_ssl_score_calls():
    L = _lib.lib()
    for name, (restype, argtypes) in _abi.SSL_SCORE_FUNCTIONS.items():
        fn = getattr(L, name)
        assert fn.restype is restype and fn.argtypes == argtypes, name
