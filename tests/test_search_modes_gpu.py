"""The opt-in search modes of a self-play engine (include/m0_gumbel.h, m0_proof.h, m0_budget.h) exclude each other and
compat.tt_merge: every ordered pair of modes and every mode with the position table, on an external-evaluation engine with one
slot.  Only setters and result getters are called: no search pass is launched and no network kernel runs.

For each case: the second setter is refused with the word that names what is in its way, the engine keeps the mode it had (its
result call answers, the refused mode's says "not set"), and once a search has begun no setter is taken any more."""
import itertools

import pytest

from oracle import chess_py as ch
from tests.test_search_gpu import MCTS

pytestmark = pytest.mark.gpu

# mode: (setter, result getter, the word the other setters name it by, a key of its result and its value before the search ends)
MODES = {
    "gumbel": ("set_gumbel", "search_gumbel_result", "Gumbel", "pick", -1),
    "proof": ("set_proof", "search_proof_result", "proof search", "pick", -1),
    "budget": ("set_budget", "search_budget_result", "budget", "forced_descents", -1),
}
BASE = {"seed": 1, "mcts": dict(MCTS, inference_batch_size=8), "selfplay": {"num_simulations": 8}}


def _engine(compat=None):
    from matrix0_amd import engine as eng
    return eng.SelfplayEngine(None, eng.selfplay_cfg_from_dict(BASE, concurrent_games=1, compat=compat))


def _check_modes(e, on):
    """The engine is in mode `on` (None: in none): that mode's result call answers, the others say "not set"."""
    for name, (_, getter, _, key, unfinished) in MODES.items():
        if name == on:
            assert getattr(e, getter)(0)[key] == unfinished
        else:
            with pytest.raises(RuntimeError, match="not set"):
                getattr(e, getter)(0)


def _check_closed_after_begin(e):
    e.search_begin(0, ch.START_FEN, 8, False, 0)
    for setter, *_ in MODES.values():
        with pytest.raises(RuntimeError, match="before the first"):
            getattr(e, setter)()


@pytest.mark.parametrize("first,second", list(itertools.permutations(MODES, 2)))
def test_a_mode_refuses_an_engine_in_another(first, second):
    e = _engine()
    getattr(e, MODES[first][0])()
    with pytest.raises(ValueError, match=MODES[first][2]):
        getattr(e, MODES[second][0])()
    if second == "proof":                       # taking the proof search back is refused like setting it
        with pytest.raises(ValueError, match=MODES[first][2]):
            e.set_proof(False)
    _check_modes(e, first)
    _check_closed_after_begin(e)
    _check_modes(e, first)
    e.close()


@pytest.mark.parametrize("mode", list(MODES))
def test_a_mode_refuses_the_position_table(mode):
    e = _engine(compat={"tt_merge": True})
    with pytest.raises(ValueError, match="tt_merge"):
        getattr(e, MODES[mode][0])()
    _check_modes(e, None)
    _check_closed_after_begin(e)
    _check_modes(e, None)
    e.close()
