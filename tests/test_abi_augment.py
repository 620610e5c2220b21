"""matrix0_amd/_abi.py against include/m0_augment.h (no GPU; the last tests need the built library): the augmentation calls and
their constants, compared name by name and type by type as tests/test_abi.py compares the main table with m0_engine.h, and the
arguments m0_augment_rows and m0_net_score_aug refuse before they touch a device."""
import ctypes as C
import os

import numpy as np

from matrix0_amd import _abi, _lib
from tests import test_abi as ta

AUGMENT_HEADER = os.path.join(os.path.dirname(ta.HEADER), "m0_augment.h")
SENTINEL = -7.0


def test_every_augment_call_is_in_the_table_with_its_types():
    h = ta.parse_header(AUGMENT_HEADER)
    assert list(h["functions"]) == list(_abi.AUGMENT_FUNCTIONS) == ["m0_augment_rows", "m0_net_score_aug", "m0_augment_bench"]
    assert not set(_abi.AUGMENT_FUNCTIONS) & (set(_abi.FUNCTIONS) | set(_abi.LIVE_FUNCTIONS) | set(_abi.SCORE_FUNCTIONS) |
                                              set(_abi.SSL_SCORE_FUNCTIONS) | set(_abi.GUMBEL_FUNCTIONS))
    for name, (ret, params) in h["functions"].items():
        restype, argtypes = _abi.AUGMENT_FUNCTIONS[name]
        assert ta.kind_of_ctype(restype) == ret == "i4", name
        assert [ta.kind_of_ctype(a) for a in argtypes] == params, name


def test_the_constants_equal_the_header_and_it_has_no_structs():
    h = ta.parse_header(AUGMENT_HEADER)
    assert not h["structs"]
    assert {k[len("M0_AUG_"):].lower(): v for k, v in h["defines"].items()} == _abi.AUGMENT_KINDS == {"none": 0, "hflip": 1, "rot180": 2}


def test_the_main_header_includes_the_augment_header_after_the_score_header():
    text = open(ta.HEADER).read()
    assert '#include "m0_augment.h"' in text and text.index('#include "m0_score.h"') < text.index('#include "m0_augment.h"')
    assert not set(_abi.AUGMENT_FUNCTIONS) & set(ta.parse_header()["functions"])
    assert "m0_augment.h" in open(os.path.join(os.path.dirname(ta.HEADER), "m0_score.h")).read()


def test_the_built_library_exports_the_augment_calls():
    L = _lib.lib()
    for name, (restype, argtypes) in _abi.AUGMENT_FUNCTIONS.items():
        fn = getattr(L, name)
        assert fn.restype is restype and fn.argtypes == argtypes, name


def _rows(B=3, P=19):
    rng = np.random.default_rng(2)
    return (rng.random((B, P, 8, 8)).astype(np.float32), rng.random((B, 4672)).astype(np.float32),
            (rng.random((B, 4672)) < 0.1).astype(np.uint8), np.array([0, 1, 2], np.uint8)[:B])


def test_augment_rows_refuses_invalid_arguments_and_touches_nothing():
    s, pi, mask, kinds = _rows()
    so, po, mo = np.full_like(s, SENTINEL), np.full_like(pi, SENTINEL), np.full_like(mask, 9)
    p = _lib.ptr

    def refused(planes=s, P=19, pi_=pi, mask_=mask, kinds_=kinds, B=3, planes_out=so, pi_out=po, mask_out=mo):
        rc = _lib.lib().m0_augment_rows(0, p(planes), P, p(pi_), p(mask_), p(kinds_), B, p(planes_out), p(pi_out), p(mask_out))
        return rc == _abi.M0_ERR_INVALID and (so == SENTINEL).all() and (po == SENTINEL).all() and (mo == 9).all() and _lib.last_error() != ""

    for null in ("planes", "pi_", "kinds_", "planes_out", "pi_out"):
        assert refused(**{null: None}), null
    for B in (0, -1):
        assert refused(B=B), B
    for P in (0, -3):
        assert refused(P=P), P
    for bad in (3, 255):
        assert refused(kinds_=np.array([0, bad, 1], np.uint8)), bad
        assert refused(kinds_=np.array([0, 1, bad], np.uint8)), bad
    assert refused(mask_out=None), "a mask without mask_out"
    assert refused(mask_=None), "mask_out without a mask"
    assert refused(planes_out=s) and refused(pi_out=pi) and refused(mask_out=mask), "in place"


def test_net_score_aug_and_the_bench_refuse_invalid_arguments_without_a_network():
    s, pi, mask, kinds = _rows()
    z = np.zeros(3, np.float32)
    rows = np.full((3, _abi.SCORE_COLS), SENTINEL, np.float32)
    opts = _abi.ScoreOpts(_abi.SCORE_MASK["legal"], 0.0, 0, 1.0)
    p = _lib.ptr
    rc = _lib.lib().m0_net_score_aug(None, p(s), p(pi), p(z), p(mask), p(kinds), 3, C.byref(opts), p(rows))
    assert rc == _abi.M0_ERR_INVALID and (rows == SENTINEL).all()
    us, nbytes = C.c_float(0), C.c_double(0)
    for B, iters in ((0, 1), (1, 0)):
        assert _lib.lib().m0_augment_bench(0, B, iters, C.byref(us), C.byref(nbytes)) == _abi.M0_ERR_INVALID
    assert _lib.lib().m0_augment_bench(0, 1, 1, None, C.byref(nbytes)) == _abi.M0_ERR_INVALID
