"""matrix0_amd/_abi.py against include/m0_batch_weighted.h (no GPU; the last tests need the built library): the calls that give the
resident rows a weight and draw batches in proportion to it, compared name by name and type by type as tests/test_abi.py compares
the main table with m0_engine.h.  include/m0_batch.h and include/m0_batch_ssl.h and their tables stay as they were
(tests/test_abi_batch.py, tests/test_abi_batch_ssl.py)."""
import ctypes as C
import os

import numpy as np

from matrix0_amd import _abi, _lib
from tests import test_abi as ta

INCLUDE = os.path.dirname(ta.HEADER)
HEADER = os.path.join(INCLUDE, "m0_batch_weighted.h")
NAMES = ["m0_rowstore_set_weights", "m0_rowstore_fill_weights", "m0_rowstore_scale_weights", "m0_rowstore_get_weights",
         "m0_rowstore_weights_info", "m0_rowstore_sample", "m0_rowstore_batch_sampled", "m0_net_score_resident", "m0_weight_from_score"]
# include/m0_batch.h as it was before this header existed: its calls with their parameter kinds, and its constants
BATCH_H = {
    "m0_rowstore_create": ("ptr", ["i4", "i4"]),
    "m0_rowstore_destroy": ("void", ["ptr"]),
    "m0_rowstore_append": ("i4", ["ptr", "ptr", "ptr"]),
    "m0_rowstore_evict": ("i4", ["ptr", "i8"]),
    "m0_rowstore_info": ("i4", ["ptr", "ptr"]),
    "m0_rowstore_batch": ("i4", ["ptr", "ptr", "ptr", "i4", "ptr", "ptr", "ptr", "ptr", "i4", "ptr"]),
    "m0_rowstore_batch_host": ("i4", ["ptr", "ptr", "ptr", "i4", "ptr", "ptr", "ptr", "ptr"]),
    "m0_rowstore_bench": ("i4", ["i4", "i4", "i4", "ptr", "ptr", "ptr"]),
}


def test_every_call_is_in_the_table_with_its_types():
    h = ta.parse_header(HEADER)
    assert list(h["functions"]) == list(_abi.BATCH_WEIGHTED_FUNCTIONS) == NAMES
    for name, (ret, params) in h["functions"].items():
        restype, argtypes = _abi.BATCH_WEIGHTED_FUNCTIONS[name]
        assert ta.kind_of_ctype(restype) == ret == "i4", name
        assert [ta.kind_of_ctype(a) for a in argtypes] == params, name
    assert list(h["structs"]) == list(_abi.BATCH_WEIGHTED_STRUCTS) == ["m0_weight_rule"]
    assert h["structs"]["m0_weight_rule"] == [(f, "f4") for f in ("policy", "kl", "value", "floor", "cap")]
    assert [(f, ta.kind_of_ctype(t)) for f, t in _abi.WeightRule._fields_] == h["structs"]["m0_weight_rule"]
    assert h["defines"] == {"M0_WEIGHT_MAX": _abi.WEIGHT_MAX, "M0_WEIGHT_ONE_TICKS": _abi.WEIGHT_ONE_TICKS,
                            "M0_WEIGHT_ROWS_MAX": _abi.WEIGHT_ROWS_MAX, "M0_WEIGHTS_INFO": len(_abi.WEIGHTS_INFO)}
    assert (_abi.WEIGHT_MAX, _abi.WEIGHT_ONE_TICKS, _abi.WEIGHT_ROWS_MAX, len(_abi.WEIGHTS_INFO)) == (65536, 2 ** 24, 2 ** 23, 4)
    # a sum of ticks stays below 2^63
    assert _abi.WEIGHT_MAX * _abi.WEIGHT_ONE_TICKS * _abi.WEIGHT_ROWS_MAX == 2 ** 63
    # the sampled batch is the SSL batch without its ids, with the draw in front and the draw's outputs behind
    ssl = _abi.BATCH_SSL_FUNCTIONS["m0_rowstore_batch_ssl"][1]
    new = _abi.BATCH_WEIGHTED_FUNCTIONS["m0_rowstore_batch_sampled"][1]
    assert new == [_abi.vp, _abi.i32, _abi.u64, _abi.u64, _abi.i32] + ssl[2:3] + ssl[4:10] + [_abi.vp, _abi.vp] + ssl[10:]
    # what the header must say in words: why ticks, and the one unspecified outcome
    text = " ".join(open(HEADER).read().split())
    assert "INDEPENDENT OF THE ORDER OF SUMMATION" in text and "ONE OF ITS VALUES IS STORED" in text
    assert "go on ONE stream" in text


def test_the_new_names_sit_in_no_other_table_and_the_header_behind_the_ssl_one():
    others = (set(_abi.FUNCTIONS) | set(_abi.LIVE_FUNCTIONS) | set(_abi.SCORE_FUNCTIONS) | set(_abi.SSL_SCORE_FUNCTIONS) |
              set(_abi.GUMBEL_FUNCTIONS) | set(_abi.AUGMENT_FUNCTIONS) | set(_abi.PROOF_FUNCTIONS) | set(_abi.ROWPACK_FUNCTIONS) |
              set(_abi.BATCH_FUNCTIONS) | set(_abi.BATCH_SSL_FUNCTIONS) | set(_abi.BUDGET_FUNCTIONS))
    assert not set(NAMES) & others
    text = open(ta.HEADER).read()
    assert (0 < text.index('#include "m0_batch.h"') < text.index('#include "m0_batch_ssl.h"') <
            text.index('#include "m0_batch_weighted.h"'))
    assert text.count('#include "m0_batch_weighted.h"') == 1
    assert not set(NAMES) & set(ta.parse_header()["functions"])
    for older in ("m0_batch.h", "m0_batch_ssl.h", "m0_score.h"):
        h = ta.parse_header(os.path.join(INCLUDE, older))
        assert not set(NAMES) & set(h["functions"]) and not [d for d in h["defines"] if d.startswith("M0_WEIGHT")], older


def test_m0_batch_h_is_what_it_was():
    h = ta.parse_header(os.path.join(INCLUDE, "m0_batch.h"))
    assert h["functions"] == BATCH_H and list(h["functions"]) == list(BATCH_H) == list(_abi.BATCH_FUNCTIONS)
    assert h["defines"] == {"M0_ROWSTORE_HOST": -1, "M0_ROWSTORE_INFO": 6} and not h["structs"]
    for name, (ret, params) in BATCH_H.items():
        restype, argtypes = _abi.BATCH_FUNCTIONS[name]
        assert ta.kind_of_ctype(restype) == ret and [ta.kind_of_ctype(a) for a in argtypes] == params, name


def test_the_built_library_exports_the_calls():
    L = _lib.lib()
    for name, (restype, argtypes) in _abi.BATCH_WEIGHTED_FUNCTIONS.items():
        fn = getattr(L, name)
        assert fn.restype is restype and fn.argtypes == argtypes, name


def test_null_arguments_are_refused_with_a_message():
    L = _lib.lib()
    p = _lib.ptr
    ids, w, info = np.zeros(1, np.int64), np.ones(1, np.float32), np.full(4, -7, np.int64)
    prob = np.full(1, -7, np.float32)
    rule = _abi.WeightRule(1.0, 0.0, 0.0, 0.0, 1.0)
    s, pi, z = np.zeros(19 * 64, np.float32), np.zeros(4672, np.float32), np.zeros(1, np.float32)
    calls = [lambda h: L.m0_rowstore_set_weights(None, p(ids), p(w), 1, 0, None),
             lambda h: L.m0_rowstore_fill_weights(None, 0, 1, 1.0),
             lambda h: L.m0_rowstore_scale_weights(None, 1.0),
             lambda h: L.m0_rowstore_get_weights(None, p(ids), 1, p(w)),
             lambda h: L.m0_rowstore_weights_info(None, p(info)),
             lambda h: L.m0_rowstore_sample(None, 1, 0, 0, 0, p(ids), p(prob), 0, None),
             lambda h: L.m0_rowstore_batch_sampled(None, 1, 0, 0, 0, None, p(s), p(pi), p(z), None, None, None, p(ids), p(prob), 0, None),
             lambda h: L.m0_net_score_resident(None, h, p(ids), None, 1, None, p(s), None),
             lambda h: L.m0_weight_from_score(None, 1, C.byref(rule), p(w)),
             lambda h: L.m0_weight_from_score(p(s), 0, C.byref(rule), p(w)),
             lambda h: L.m0_weight_from_score(p(s), 1, None, p(w)),
             lambda h: L.m0_rowstore_set_weights(h, None, p(w), 1, 0, None),
             lambda h: L.m0_rowstore_set_weights(h, p(ids), p(w), 1, 1, None),          # device memory for a host store
             lambda h: L.m0_rowstore_get_weights(h, p(ids), 1, None),
             lambda h: L.m0_rowstore_weights_info(h, None),
             lambda h: L.m0_rowstore_sample(h, 1, 0, 0, 0, None, p(prob), 0, None),
             lambda h: L.m0_rowstore_sample(h, 0, 0, 0, 0, p(ids), p(prob), 0, None),
             lambda h: L.m0_rowstore_sample(h, 1, 0, 0, 0, p(ids), p(prob), 1, None),   # device outputs of a host store
             lambda h: L.m0_rowstore_sample(h, 1, 0, 0, 0, p(ids), p(prob), 0, None),   # nothing is resident
             lambda h: L.m0_rowstore_batch_sampled(h, 1, 0, 0, 0, None, p(s), p(pi), p(z), None, None, None, p(ids), p(prob), 0, None)]
    h = L.m0_rowstore_create(_abi.ROWSTORE_HOST, 0)
    try:
        for k, call in enumerate(calls):
            assert call(h) == _lib.M0_ERR_INVALID and _lib.last_error(), k
    finally:
        L.m0_rowstore_destroy(h)
    assert (prob == -7).all() and (info == -7).all() and not ids.any()
