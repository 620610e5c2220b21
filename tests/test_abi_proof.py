"""matrix0_amd/_abi.py against include/m0_proof.h (no GPU; one test needs the built library): the proof search's calls, constants
and its struct of analysis proofs, compared name by name and type by type as tests/test_abi.py compares the main table with
m0_engine.h."""
import ctypes as C
import os

from matrix0_amd import _abi, _lib, engine as eng
from tests import test_abi as ta

PROOF_HEADER = os.path.join(os.path.dirname(ta.HEADER), "m0_proof.h")


def test_every_proof_call_is_in_the_table_with_its_types():
    h = ta.parse_header(PROOF_HEADER)
    assert list(h["functions"]) == list(_abi.PROOF_FUNCTIONS) == ["m0_selfplay_set_proof", "m0_search_proof_result",
                                                                  "m0_analysis_last_proof", "m0_proof_combine"]
    others = (set(_abi.FUNCTIONS) | set(_abi.LIVE_FUNCTIONS) | set(_abi.SCORE_FUNCTIONS) | set(_abi.SSL_SCORE_FUNCTIONS) |
              set(_abi.GUMBEL_FUNCTIONS) | set(_abi.AUGMENT_FUNCTIONS))
    assert not set(_abi.PROOF_FUNCTIONS) & others
    for name, (ret, params) in h["functions"].items():
        restype, argtypes = _abi.PROOF_FUNCTIONS[name]
        assert ta.kind_of_ctype(restype) == ret == "i4", name
        assert [ta.kind_of_ctype(a) for a in argtypes] == params, name


def test_the_states_and_the_proof_struct_equal_the_header():
    h = ta.parse_header(PROOF_HEADER)
    assert h["defines"] == {"M0_PROOF_" + name.upper(): value for value, name in enumerate(eng.PROOF_STATES)}
    assert eng.PROOF_STATES == ["none", "win", "loss", "draw"]
    # the four fields the analysis result gains in this mode, under their names, in a struct of their own
    assert list(h["structs"]) == list(_abi.PROOF_STRUCTS) == ["m0_proof_lines"]
    fields, mirror = h["structs"]["m0_proof_lines"], _abi.ProofLines._fields_
    assert [f for f, _ in fields] == [f for f, _ in mirror] == ["proof", "proof_plies", "line_proof", "line_proof_plies"]
    lines = ("array", "i4", eng.AN_MAX_LINES)
    assert [k for _, k in fields] == [ta.kind_of_ctype(t) for _, t in mirror] == ["i4", "i4", lines, lines]
    assert C.sizeof(_abi.ProofLines) == 8 + 8 * eng.AN_MAX_LINES


def test_the_main_header_includes_the_proof_header():
    assert '#include "m0_proof.h"' in open(ta.HEADER).read()
    main = ta.parse_header()
    assert not set(_abi.PROOF_FUNCTIONS) & set(main["functions"]) and "m0_proof_lines" not in main["structs"]


def test_the_built_library_exports_the_proof_calls():
    L = _lib.lib()
    for name, (restype, argtypes) in _abi.PROOF_FUNCTIONS.items():
        fn = getattr(L, name)
        assert fn.restype is restype and fn.argtypes == argtypes, name


def test_the_result_dict_carries_the_proofs():
    r, p = eng.AnalysisResult(), _abi.ProofLines()
    r.nlines = 2
    p.proof, p.proof_plies = 1, 3
    p.line_proof[0], p.line_proof_plies[0], p.line_proof[1], p.line_proof_plies[1] = 1, 3, 2, 4
    d = eng.analysis_result_to_dict(r, p)
    assert (d["proof"], d["proof_plies"]) == ("win", 3)
    assert [(ln["proof"], ln["proof_plies"]) for ln in d["lines"]] == [("win", 3), ("loss", 4)]
    assert "proof" not in eng.analysis_result_to_dict(r) and "proof" not in eng.analysis_result_to_dict(r)["lines"][0]
