"""matrix0_amd/_abi.py against include/m0_budget.h (no GPU; the last test needs the built library): the calls of the self-play
budget mix and its options struct, compared name by name and type by type as tests/test_abi.py compares the main table with
m0_engine.h."""
import ctypes as C
import os

from matrix0_amd import _abi, _lib
from tests import test_abi as ta

BUDGET_HEADER = os.path.join(os.path.dirname(ta.HEADER), "m0_budget.h")


def test_every_budget_call_is_in_the_table_with_its_types():
    h = ta.parse_header(BUDGET_HEADER)
    assert list(h["functions"]) == list(_abi.BUDGET_FUNCTIONS) == [
        "m0_selfplay_set_budget", "m0_search_budget_result", "m0_game_record_budget", "m0_selfplay_budget_stats",
        "m0_budget_is_full", "m0_budget_forced", "m0_budget_prune"]
    others = (set(_abi.FUNCTIONS) | set(_abi.LIVE_FUNCTIONS) | set(_abi.SCORE_FUNCTIONS) | set(_abi.SSL_SCORE_FUNCTIONS) |
              set(_abi.GUMBEL_FUNCTIONS) | set(_abi.AUGMENT_FUNCTIONS) | set(_abi.PROOF_FUNCTIONS) | set(_abi.ROWPACK_FUNCTIONS) |
              set(_abi.BATCH_FUNCTIONS))
    assert not set(_abi.BUDGET_FUNCTIONS) & others
    for name, (ret, params) in h["functions"].items():
        restype, argtypes = _abi.BUDGET_FUNCTIONS[name]
        assert ta.kind_of_ctype(restype) == ret == "i4", name
        assert [ta.kind_of_ctype(a) for a in argtypes] == params, name


def test_the_options_struct_equals_the_header():
    h = ta.parse_header(BUDGET_HEADER)
    assert list(h["structs"]) == list(_abi.BUDGET_STRUCTS) == ["m0_budget_cfg"]
    fields = h["structs"]["m0_budget_cfg"]
    mirror = _abi.BudgetCfg._fields_
    assert [f for f, _ in fields] == [f for f, _ in mirror] == ["full_prob", "fast_simulations", "forced_k", "prune_targets"]
    assert [k for _, k in fields] == [ta.kind_of_ctype(t) for _, t in mirror] == ["f8", "i4", "f8", "i4"]
    assert C.sizeof(_abi.BudgetCfg) == 32
    assert not h["defines"]


def test_the_main_header_includes_the_budget_header_and_keeps_its_own_structs():
    assert '#include "m0_budget.h"' in open(ta.HEADER).read()
    main = ta.parse_header()
    assert "m0_budget_cfg" not in main["structs"] and not set(_abi.BUDGET_FUNCTIONS) & set(main["functions"])
    # the game record itself did not change: the per-ply budget travels beside it (m0_game_record_budget)
    assert [f for f, _ in main["structs"]["m0_game_record"]] == [f[0] for f in _abi.GameRecord._fields_]
    assert "full" not in [f[0] for f in _abi.GameRecord._fields_]


def test_the_built_library_exports_the_budget_calls():
    L = _lib.lib()
    for name, (restype, argtypes) in _abi.BUDGET_FUNCTIONS.items():
        fn = getattr(L, name)
        assert fn.restype is restype and fn.argtypes == argtypes, name
