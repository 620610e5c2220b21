"""The cases of tests/draw_rule_cases.py with the oracle alone, no GPU: every scripted history is legal and reversible and puts
the repeated position where the case says; every oracle search meets the rule its case is about, often enough and next to
enough network leaves; and every mutant (a threshold moved by one, a rule dropped) and control input (a history cut short)
changes the oracle's result.  This is what keeps tests/test_draw_rules_gpu.py from passing on a case that never meets its rule.

The conditions are minimums.  If one fails after a change to the oracle or an evaluator, choose another game id or evaluator
seed for the case; do not lower the condition.  "Network leaves" are counted as evaluations, the root's own included, as the
figures the cases were chosen by counted them."""
import pytest

from oracle import chess_py as ch
from tests import draw_rule_cases as dc
from tests import proof_ref as pr

START_KEY = ch.Board(ch.START_FEN)._transposition_key()
BUDGETS = [(8, True), (8, False), (1, True)]                 # leaves per pass, virtual loss: the runs of group 2


def _kinds(want):
    return want["oracle"].kinds


def _differs(a, b):
    """Two oracle searches that a comparison of root visit counts tells apart."""
    return a["counts"] != b["counts"]


# ---------------------------------------------------------------- histories ----------------------------------------------------------------
@pytest.mark.parametrize("moves,length,at", [(dc.MOVES_2A, 12, [0, 4, 8]), (dc.MOVES_2B, 8, [0, 4]), (dc.MOVES_2C, 71, [0, 4, 64, 68]),
                                             (dc.MOVES_2D, 135, [0, 64, 128, 132]), (dc.MOVES_KEPT + dc.S[2:], 12, [0, 4, 8])])
def test_histories_are_legal_reversible_and_place_the_start_position(moves, length, at):
    board, window, reversible = dc.replay(ch.START_FEN, moves)
    assert all(reversible) and len(window) == length == len(moves) == board.halfmove_clock
    assert [i for i, k in enumerate(window) if k == START_KEY] == at
    assert not board.is_game_over()
    # the fifth occurrence of the start position is within reach of the search: one move away, or one round of the knights
    b = board.copy()
    for u in (dc.S[3:] if board._transposition_key() != START_KEY else dc.S):
        assert not b.is_game_over()
        b.push(ch.Move.from_uci(u))
    assert b._transposition_key() == START_KEY
    assert b.is_fivefold_repetition() == (len(at) + (board._transposition_key() == START_KEY) >= 4)
    assert b.is_repetition(len(at) + 1 + (board._transposition_key() == START_KEY))


def test_the_long_windows_need_every_trip_of_64_entries():
    """2c: occurrences in the first and the second 64 entries; 2d: in all three.  With only the last 64 (2d: 128, 64) moves as
    history, or none, no leaf is a fifth occurrence any more."""
    assert 64 < len(dc.MOVES_2C) <= 128 < 130 <= len(dc.MOVES_2D) <= 149
    for name, keeps in (("2c", (64, 0)), ("2d", (128, 64, 0))):
        full = dc.oracle_run(name)
        print(dc.kinds_line(name, full))
        assert _kinds(full)["5fold"] >= 1 and full["evals"] >= 10, name
        for keep in keeps:
            cut = dc.oracle_run(name, keep=keep)
            print(dc.kinds_line(f"{name}, last {keep} moves as history", cut))
            assert ch.Board(dc.CASES[name].root_fen(keep)).halfmove_clock == len(dc.CASES[name].moves) - keep
            assert _kinds(cut)["5fold"] == 0 and _differs(cut, full), (name, keep)
            assert cut["evals"] != full["evals"], (name, keep)


def test_the_window_that_overflows_is_over_by_the_clock_first():
    """2e: 200 reversible plies.  The root is drawn by rule twice over.  The engine's window holds the last 192 entries only,
    and no leaf can tell: a leaf reached by reversible moves alone has a clock of 201 or more and is a 75-move draw first, with
    the same value; behind an irreversible move (clock 0) the window is not consulted and nothing in it can recur."""
    board, window, reversible = dc.replay(ch.START_FEN, dc.MOVES_2E)
    assert all(reversible) and len(window) == 200 > 192 and board.halfmove_clock == 200
    assert board.is_game_over() and board.is_seventyfive_moves() and board.is_fivefold_repetition() and board.legal_moves
    quiet = 0
    for m in board.legal_moves:
        b = board.copy()
        b.push(m)
        if b.halfmove_clock == 201:
            quiet += 1
            assert dc.Counting.kind_of(b) == "75"
        else:
            assert b.halfmove_clock == 0 and b._transposition_key() not in window and not b.is_game_over()
    assert quiet == 4                                        # the knights' moves


# ---------------------------------------------------------------- group 1 ----------------------------------------------------------------
@pytest.mark.parametrize("vl", [True, False])
def test_the_75_move_rule_is_met_at_depths_one_and_two(vl):
    for name in ("1b", "1c"):
        want = dc.oracle_run(name, 8, vl)
        print(dc.kinds_line(f"{name} vl={vl}", want))
        assert _kinds(want)["75"] >= 5 and want["evals"] >= 10, name
        assert sum(_kinds(want).values()) == _kinds(want)["75"]                  # no other rule ends a leaf here
    far = dc.oracle_run("1a", 8, vl)                                             # clock 147: the rule is three plies away
    print(dc.kinds_line(f"1a vl={vl}", far))                                     # recorded, no minimum
    assert not ch.Board(dc.CASES["1c"].fen).is_game_over()


@pytest.mark.parametrize("vl", [True, False])
@pytest.mark.parametrize("name,mutant", [("1b", m) for m in sorted(dc.MUTANTS_75)] + [("1c", "75 at 151"), ("1c", "75 dropped")])
def test_the_75_move_mutants_change_the_search(name, mutant, vl):
    """(A threshold of 149 cannot show from 1c's root: its clock is 149 already, every quiet child has 150 either way.)"""
    true, bent = dc.oracle_run(name, 8, vl), dc.oracle_run(name, 8, vl, mutant=mutant)
    print(f"{name} vl={vl} {mutant}: {bent['oracle'].ended} leaves ended (true rules: {true['oracle'].terminal_leaves})")
    assert _differs(true, bent)


def test_the_true_predicate_is_the_oracles_game_over_test():
    """The mutant harness itself: with (150, 5) it reproduces the oracle's own searches."""
    for name in ("1b", "2a", "2c", "3a"):
        true, same = dc.oracle_run(name), dc.oracle_run(name, mutant="true rules")
        assert same["counts"] == true["counts"] and same["evals"] == true["evals"] and same["lines"] == true["lines"], name
        assert same["oracle"].ended == true["oracle"].terminal_leaves, name


# ---------------------------------------------------------------- group 2 ----------------------------------------------------------------
@pytest.mark.parametrize("L,vl", BUDGETS)
@pytest.mark.parametrize("name", ["2a", "2b"])
def test_fivefold_leaves_that_need_the_path(name, L, vl):
    """No position is in the window of 2a more than three times, of 2b more than twice: every fivefold leaf counts one (2b:
    two) of the positions the descent itself went through.  Dropping the rule is therefore what an engine without the path
    scan would do, and it changes the evaluations of every run."""
    _, window, _ = dc.replay(ch.START_FEN, dc.CASES[name].moves)
    assert max(window.count(k) for k in window) == (3 if name == "2a" else 2)
    want = dc.oracle_run(name, L, vl)
    print(dc.kinds_line(f"{name} L={L} vl={vl}", want))
    assert _kinds(want)["5fold"] >= 5 and want["evals"] >= 10, name
    assert sum(_kinds(want).values()) == _kinds(want)["5fold"]
    for mutant in sorted(dc.MUTANTS_5FOLD):
        bent = dc.oracle_run(name, L, vl, mutant=mutant)
        print(f"    {mutant}: {bent['oracle'].ended} leaves ended, {bent['evals']} evaluations")
        assert bent["oracle"].ended != want["oracle"].terminal_leaves and bent["evals"] != want["evals"], mutant
    if name == "2a" and (L, vl) == (8, True):
        for mutant in ("fold at 4", "fold at 6", "fold dropped"):
            assert _differs(want, dc.oracle_run(name, L, vl, mutant=mutant)), mutant


# ---------------------------------------------------------------- groups 3 and 4 ----------------------------------------------------------------
def test_insufficient_material_is_reached_by_a_capture_inside_the_tree():
    want = dc.oracle_run("3a")
    print(dc.kinds_line("3a", want))
    assert not ch.Board(dc.KBKN).is_insufficient_material()
    assert _kinds(want)["insufficient"] >= 5 and want["evals"] >= 10


def test_the_75_move_draw_comes_ahead_of_the_table():
    from tests import tb_search_util as su
    from tests import tb_util as tu
    board = ch.Board(dc.TB_149)
    assert su.py_probe(board, tu.ref_tables()) is None and board.halfmove_clock == 149 and not board.is_game_over()
    for m in board.legal_moves:                              # every child: a table win for White, and drawn by the clock
        b = board.copy()
        b.push(m)
        hit = su.py_probe(b, tu.ref_tables())
        assert hit is not None and hit[0] == -1 and b.is_seventyfive_moves(), m
    late, _ = dc.oracle_tb(dc.TB_149)
    early, _ = dc.oracle_tb(dc.RIGHT_LEFT)
    print(f"clock 149: {late.kinds}, {late.tb_leaves} table leaves; clock 0: {early.kinds}, {early.tb_leaves} table leaves")
    assert late.tb_leaves == 0 and late.kinds["75"] >= 5
    assert early.tb_leaves >= 10 and early.terminal_leaves == 0


# ---------------------------------------------------------------- group 5 ----------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 16])
def test_the_75_move_rule_proves_a_draw(L):
    o, want = dc.oracle_proof("1c", L)
    drawn = [c for c in want["children"] if c == (pr.DRAW, 0)]
    print(f"L={L}: {len(drawn)} of {len(want['children'])} root children drawn, root {want['state']}, closest scan {o.min_gap}")
    assert len(drawn) >= 3 and o.min_gap >= 1e-4
    assert want["state"] == pr.NONE                          # the pawn moves and captures go on


@pytest.mark.parametrize("L", [8, 1])
def test_a_fivefold_leaf_proves_nothing(L):
    o, want = dc.oracle_proof("2a", L)
    plain = dc.oracle_run("2a", L, True)
    print(f"L={L}: {o.kinds}, {o.evals} evaluations")
    assert not o.proofs and o.kinds["5fold"] >= 5
    # ... and is visited again: the search is the plain one
    assert [c.n for c in want["root"].children.values()] == plain["counts"] and o.evals == plain["evals"]
    assert o.kinds == plain["oracle"].kinds


# ---------------------------------------------------------------- modes ----------------------------------------------------------------
def test_the_position_table_runs_meet_their_rules():
    """compat.tt_merge: the history is played in (see draw_rule_cases).  2b is the negative row: no fivefold leaf."""
    seen = {}
    for name in ("1b", "2a", "2b", "2c"):
        want = dc.oracle_played_tt(name)
        print(dc.kinds_line(f"{name}, position table", want))
        seen[name] = want
    assert _kinds(seen["1b"])["75"] >= 5 and seen["1b"]["evals"] >= 10
    assert _kinds(seen["2a"])["5fold"] >= 5 and seen["2a"]["evals"] >= 10
    assert _kinds(seen["2c"])["5fold"] >= 1
    assert _kinds(seen["2b"])["5fold"] == 0 and seen["2b"]["evals"] == 129


def test_the_gumbel_runs_meet_their_rules():
    for name, kind in (("1c", "75"), ("2a", "5fold")):
        o, want, _ = dc.oracle_played_gumbel(name)
        print(f"{name}, Gumbel root: {o.kinds}, {o.evals} evaluations, closest root decision {o.min_gap}")
        assert o.kinds[kind] >= 5 and o.miss == 0 and o.min_gap >= 1e-4, name


def test_the_kept_tree_sees_the_longer_window():
    """Continuing the tree of S S g1f3 g8f6 by f3g1 f6g8 gives 2a's root.  The oracle's continued search on the history differs
    from the one on a tree that was started from the bare FEN of the same position."""
    with_history, bare = dc.oracle_kept(True), dc.oracle_kept(False)
    for tag, (n_before, want) in (("history", with_history), ("bare FEN", bare)):
        print(f"kept tree, {tag}: {n_before} visits kept, {want['oracle'].kinds}, {want['evals']} evaluations")
    assert with_history[0] > 0 and bare[0] > 0
    assert with_history[1]["oracle"].kinds["5fold"] >= 5 and with_history[1]["oracle"].kinds != bare[1]["oracle"].kinds
    assert with_history[1]["counts"] != bare[1]["counts"]
    assert with_history[1]["lines"] != bare[1]["lines"] and with_history[1]["evals"] != bare[1]["evals"]


def test_the_slot_jobs_meet_their_rules():
    for name, uid in dc.SLOT_JOBS:
        want = dc.oracle_slot_job(name, uid)
        print(dc.kinds_line(f"{name} as slot job {uid}", want))
        assert _kinds(want)[dc.SLOT_RULE[name]] >= 5 and want["evals"] >= 10, name
    # the two that take the slots first have the longest windows, and run as long as each other
    (a, _), (b, _) = dc.SLOT_JOBS[:2]
    assert min(len(dc.CASES[a].moves), len(dc.CASES[b].moves)) > max(len(dc.CASES[n].moves) for n, _ in dc.SLOT_JOBS[2:])
    assert dc.CASES[a].sims == dc.CASES[b].sims
