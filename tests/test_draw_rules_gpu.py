"""The draw rules of a search leaf on the GPU (leaf_terminal, csrc/tree_select.hip: the 75-move rule, fivefold repetition on the
descent's path and in the game's history window, insufficient material, all ahead of the table probe; leaf_proof,
csrc/tree_proof.h) against the oracle's MCTS, on the cases of tests/draw_rule_cases.py.  tests/test_draw_rules.py shows on the
CPU that every case meets its rule and that bending the rule changes the oracle's result.

The engine is the analysis engine with the caller's evaluator, which takes a FEN and the moves that led to it.  The modes only
a self-play engine's split-step search has (position table, Gumbel root, the proof results per root child) run there; where
they need a history it is played in, one search of one simulation per ply (draw_rule_cases.oracle_played_tt).

Compared as tests/test_analysis_gpu._check and tests/test_search_gpu._compare compare: status, legal moves, root visits,
evaluations, moves, policy indices, visit counts (of every root child) and principal variations identical; priors, q and the
root's q within 1e-6; proof states and plies identical.

What this pins in leaf_terminal: without the 75-move line every case of group 1 changes its visit counts (the oracle under the
`75 dropped` mutant); without the path scan 2a and 2b meet no fivefold leaf (no position is in their windows four times) and
change their evaluations; with one trip of the window loop 2c and 2d lose the occurrences at entries 64.. and 128.. and search as
with the history cut to its last 64 moves, which the oracle shows to be another search.  Each of the three was also seen: on
scratch builds of the kernel with that one change, the tests named here failed (2e, which no clip can change, kept passing)."""
import functools

import numpy as np
import pytest

from oracle import chess_py as ch
from tests import draw_rule_cases as dc
from tests import gumbel_ref as gr
from tests import proof_ref as pr
from tests import test_gumbel_gpu as tgg
from tests import test_proof_gpu as tpg
from tests import test_tb_search_gpu as tbs
from tests.fake_net import FakeNet
from tests.test_analysis_gpu import MULTIPV, PV_LEN, SIMS, _check, _oracle_run
from tests.test_search_gpu import MCTS, _compare, _engine as _split_engine, _run_engine_search
from tests.test_tb_search_gpu import tb3                     # noqa: F401  (the module fixture: the 3-man tables, built once)

pytestmark = pytest.mark.gpu


def _analyzer(infer_np, slots, L, sims, vl=True, prove=False):
    """AnalyzerExt with what it does not pass through: virtual loss off, the proof search; and with every root child's visit
    count in its results."""
    from matrix0_amd import analysis
    from matrix0_amd import engine as eng

    class DirectAnalyzer(analysis.AnalyzerExt):
        def __init__(self):
            self.infer_np, self.multipv, self._tb_owned = infer_np, MULTIPV, None
            self.cfg = eng.selfplay_cfg_from_dict({"seed": dc.SEED, "mcts": dict(MCTS, inference_batch_size=L),
                                                   "selfplay": {"num_simulations": sims}}, concurrent_games=slots,
                                                  virtual_loss_active=vl, compat=None, record_games=False)
            self.engine = eng.AnalysisExtEngine(self.cfg, multipv=MULTIPV, pv_len=PV_LEN, dirichlet=False)
            self.engine.keep_visits(True)
            self.engine.poll = functools.partial(self.engine.poll, visits=True)
            if prove:
                self.engine.set_proof()

    return DirectAnalyzer()


def _same(got, want, sims, tag):
    """_check of tests/test_analysis_gpu (whose own budget is 64 simulations: the result's is asserted here), and the visit
    count of every root child, not only of the best lines."""
    assert got["sims"] == sims, tag
    _check(dict(got, sims=SIMS), want, tag)
    assert got["policy_idx"].tolist() == want["idx"] and got["visits"].tolist() == want["counts"], tag


def _equal_results(a, b, tag):
    """Two results of the analysis engine, every field, floats included."""
    arrays = ("policy_idx", "visits")
    for key in arrays:
        assert np.array_equal(a[key], b[key]), (tag, key)
    assert {k: v for k, v in a.items() if k not in arrays} == {k: v for k, v in b.items() if k not in arrays}, tag


def _search_case(an, name, keep=None):
    case = dc.CASES[name]
    return an.analyse([case.position(keep)], case.sims, ids=[case.uid])[0]


# ---------------------------------------------------------------- group 1 ----------------------------------------------------------------
@pytest.mark.parametrize("vl", [True, False])
def test_the_75_move_rule_ends_a_leaf(vl):
    """Clock 147, 148, 149 at the root: the rule three plies away (few leaves, if any), two and one."""
    an = _analyzer(dc.fake_net().infer_np, 1, 8, 64, vl)
    got = {name: _search_case(an, name) for name in ("1a", "1b", "1c")}
    an.close()
    for name, g in got.items():
        want = dc.oracle_run(name, 8, vl)
        print(dc.kinds_line(f"{name} vl={vl}", want))
        _same(g, want, 64, (name, vl))


# ---------------------------------------------------------------- group 2 ----------------------------------------------------------------
@pytest.mark.parametrize("L,vl", [(8, True), (8, False), (1, True)])
def test_fivefold_leaves_count_the_positions_of_the_descent(L, vl):
    """2a, 2b: the window alone holds the repeated position three times and twice."""
    an = _analyzer(dc.shuffle_net().infer_np, 1, L, 128, vl)
    got = {name: _search_case(an, name) for name in ("2a", "2b")}
    an.close()
    for name, g in got.items():
        want = dc.oracle_run(name, L, vl)
        print(dc.kinds_line(f"{name} L={L} vl={vl}", want))
        _same(g, want, 128, (name, L, vl))


@pytest.mark.parametrize("name,keeps", [("2c", (None, 64, 0)), ("2d", (None, 128, 64, 0))])
def test_fivefold_leaves_count_every_entry_of_a_long_window(name, keeps):
    """Windows of 71 and 135 entries: occurrences beyond the first 64 and the first 128.  The controls -- only the last 128 / 64
    moves as history, the bare FEN -- are other searches, in the oracle and in the engine."""
    an = _analyzer(dc.fake_net().infer_np, 1, 8, 128)
    got = [_search_case(an, name, keep) for keep in keeps]
    an.close()
    for keep, g in zip(keeps, got):
        want = dc.oracle_run(name, keep=keep)
        print(dc.kinds_line(f"{name}, history {keep}", want))
        _same(g, want, 128, (name, keep))
    for g in got[1:]:
        assert g["visits"].tolist() != got[0]["visits"].tolist() and g["evals"] != got[0]["evals"]


def test_a_history_longer_than_the_window_the_engine_keeps():
    """2e, 200 reversible plies: the root is over by rule and searched all the same (test_analysis_gpu._oracle_run, its branch
    for such roots).  The engine keeps the last 192 entries of the window and must still equal the oracle: a leaf behind
    reversible moves alone has a clock of at least 201 and is a 75-move draw before the repetition count is taken, with the same
    value; behind an irreversible move the window is not consulted (tests/test_draw_rules.py asserts both)."""
    an = _analyzer(dc.fake_net().infer_np, 1, 8, SIMS)
    got = an.analyse([(ch.START_FEN, dc.MOVES_2E)], SIMS, ids=[12])[0]
    an.close()
    want = _oracle_run(ch.START_FEN, dc.MOVES_2E, 12, False, 0.5)
    _check(got, want, "2e")
    assert got["visits"].tolist() == want["counts"]
    assert want["evals"] <= SIMS - 4                          # the knights' moves ended at once, again and again


# ---------------------------------------------------------------- group 3 ----------------------------------------------------------------
def test_insufficient_material_behind_a_capture():
    an = _analyzer(dc.fake_net().infer_np, 1, 8, 64)
    got = _search_case(an, "3a")
    an.close()
    _same(got, dc.oracle_run("3a"), 64, "3a")


# ---------------------------------------------------------------- group 4 ----------------------------------------------------------------
@pytest.mark.parametrize("fen", [dc.TB_149, dc.RIGHT_LEFT])
def test_the_75_move_draw_comes_ahead_of_the_table(tb3, fen):                    # noqa: F811
    """Every child of the root is a table win; with the clock at 149 it is a 75-move draw first, worth draw_penalty, and no
    leaf is taken from the tables.  With the clock at 0 every leaf is."""
    e = tbs._search_engine(1, 8, True, tb3)
    e.search_begin(0, fen, 64, False, 77)
    res = tbs._run_search(e, FakeNet(seed=3, sharp=8.0), 1)[0]
    evals, leaves = int(e.stats()["evals"]), e.tb_leaves()
    e.close()
    o, rq = dc.oracle_tb(fen)
    tbs._compare(res, o, rq, fen)
    assert (evals, leaves) == (o.evals, o.tb_leaves)
    assert leaves == (0 if fen == dc.TB_149 else 64)
    if fen == dc.TB_149:
        assert abs(res["root_q"] + MCTS["draw_penalty"]) <= 1e-9                  # 64 draws, seen from the root's side


# ---------------------------------------------------------------- group 5 ----------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 16])
def test_the_75_move_rule_proves_a_draw(L):
    case = dc.CASES["1c"]
    o, want = dc.oracle_proof("1c", L)
    assert o.min_gap >= tpg.MIN_GAP, f"a children scan decided by {o.min_gap}: choose another game id"
    e = tpg._engine(1, L, case.sims, True)
    e.search_begin(0, case.fen, case.sims, False, dc.PROOF_UID["1c"])
    rows = tpg._run(e, case.net(), 1)
    res, pres, evals = e.search_result(0), e.search_proof_result(0), int(e.stats()["evals"])
    e.close()
    kids = list(want["root"].children.values())
    assert res["finished"] and res["moves"] == [c.move.uci() for c in kids]
    assert res["n"].tolist() == [c.n for c in kids] and res["root_n"] == want["root"].n == o.sims
    assert rows == o.rows and evals == o.evals
    np.testing.assert_allclose(res["prior"], [c.prior for c in kids], rtol=0, atol=1e-6)
    np.testing.assert_allclose(res["q"], [c.q for c in kids], rtol=0, atol=1e-6)
    assert list(zip(pres["child_state"], pres["child_plies"].tolist())) == want["children"]
    assert (pres["state"], pres["plies"], pres["pick"]) == (want["state"], want["plies"], want["pick"])
    assert pres["child_state"].count(pr.DRAW) >= 3


@pytest.mark.parametrize("L", [8, 1])
def test_a_fivefold_leaf_proves_nothing_and_is_visited_again(L):
    o, _ = dc.oracle_proof("2a", L)
    assert not o.proofs
    got = []
    for prove in (True, False):
        an = _analyzer(dc.shuffle_net().infer_np, 1, L, 128, prove=prove)
        got.append(_search_case(an, "2a"))
        an.close()
    on, off = got
    assert on["proof"] == pr.NONE and on["proof_plies"] == 0 and all(ln["proof"] == pr.NONE for ln in on["lines"])
    assert "proof" not in off
    for ln in on["lines"]:
        del ln["proof"], ln["proof_plies"]
    del on["proof"], on["proof_plies"]
    _equal_results(on, off, L)                                # visits, priors, q, evaluations: bit for bit
    _same(off, dc.oracle_run("2a", L, True), 128, ("2a", L))


# ---------------------------------------------------------------- modes ----------------------------------------------------------------
def _play_in(e, run, case):
    """The case's root on slot 0 of a split-step engine: its FEN, then move by move behind a search of one simulation.
    `run(e)`: the searches of the engine to their end, returns the result of slot 0."""
    e.search_begin(0, case.fen, 1 if case.moves else case.sims, False, case.uid)
    for i, u in enumerate(case.moves):
        res = run(e)
        e.search_advance(0, res["moves"].index(u), case.sims if i + 1 == len(case.moves) else 1, False)
    return int(e.stats()["evals"])


@pytest.mark.parametrize("name", ["1b", "2a", "2b", "2c"])
def test_the_rules_hold_in_the_position_table_walk(name):
    """compat.tt_merge, where the walk leaves the edge it scored for the node the table holds: the leaf's position, not the
    node, decides.  2b is the negative row: 128 simulations, no fivefold leaf, 129 evaluations."""
    case = dc.CASES[name]
    want = dc.oracle_played_tt(name)
    print(dc.kinds_line(f"{name}, position table", want))
    e, _ = _split_engine(1, 8, case.sims, compat={"tt_merge": True})
    net = case.net()
    run = lambda e: _run_engine_search(e, net, 1)[0]                              # noqa: E731
    before = _play_in(e, run, case)
    res = run(e)
    evals = int(e.stats()["evals"]) - before
    e.close()
    _compare(res, want["oracle"], None, want["root_q"])
    assert evals == want["evals"]
    if name == "2b":
        assert evals == 129


@pytest.mark.parametrize("name", ["1c", "2a"])
def test_the_rules_hold_under_the_gumbel_root(name):
    """What tests/test_gumbel_gpu.py compares; the Gumbel draws of 2a's last search follow those of the searches that played
    its history in, so its `gl` is compared with the reference's own."""
    case = dc.CASES[name]
    o, want, root_fen = dc.oracle_played_gumbel(name)
    assert o.miss == 0 and o.min_gap >= tgg.MIN_GAP, f"a root decision by {o.min_gap}: choose another game id"
    gumbel = dict(gr.DEFAULTS)
    e, _ = tgg._engine(1, 8, case.sims, True, gumbel)
    net = case.net()
    before = _play_in(e, lambda e: tgg._run(e, net, 1)[0][0], case)
    results, gresults, rows = tgg._run(e, net, 1)
    evals = int(e.stats()["evals"]) - before
    e.close()
    res, gres = results[0], gresults[0]
    kids = list(want["root"].children.values())
    assert rows == o.rows and evals == o.evals
    assert res["moves"] == [c.move.uci() for c in kids] and res["n"].tolist() == [c.n for c in kids]
    assert int(res["n"].sum()) == case.sims and gres["miss"] == 0 and gres["pick"] == want["pick"]
    np.testing.assert_allclose(res["prior"], [c.prior for c in kids], rtol=0, atol=1e-6)
    np.testing.assert_allclose(res["q"], [c.q for c in kids], rtol=0, atol=1e-6)
    np.testing.assert_allclose(gres["gl"], want["gl"], rtol=0, atol=1e-6)        # g + log(prior): the priors' float32 error
    pi, v_mix, pick, _ = gr.improve(res["prior"], res["q"], res["n"], gres["gl"], want["root_v"], gumbel["c_visit"], gumbel["c_scale"])
    np.testing.assert_allclose(gres["pi"], pi, rtol=0, atol=1e-9)
    assert abs(gres["v_mix"] - v_mix) <= 1e-9 and gres["pick"] == pick
    if not case.moves:                                        # a slot's first search: the whole comparison of that file
        o._uid = case.uid
        tgg._check(res, gres, o, want, net, root_fen, gumbel)


def _drain(e, net):
    out = {}
    for _ in range(10000):
        while (r := e.poll()) is not None:
            out[r["id"]] = r
        if e.pending() == 0:
            return out
        e.step(net.infer_np, 1)
    raise AssertionError("the searches did not end")


@pytest.mark.parametrize("history", [True, False])
def test_a_continued_search_sees_the_window_of_its_new_root(history):
    """A tree kept after 64 simulations and continued behind f3g1 f6g8: the slot is re-armed with the window of the longer
    line, and the search on the kept subtree equals the oracle's on the same history.  Without the history (the first root given
    as a bare FEN) it is another search: the oracle's results differ (tests/test_draw_rules.py), the engine equals each."""
    first, _, _ = dc.replay(ch.START_FEN, dc.MOVES_KEPT)
    n_before, want = dc.oracle_kept(history)
    an = _analyzer(dc.shuffle_net().infer_np, 1, 8, 128)
    e, net = an.engine, dc.shuffle_net()
    position = (ch.START_FEN, dc.MOVES_KEPT) if history else (first.fen(), [])
    e.submit(position[0], position[1], sims=dc.KEPT_SIMS[0], id=dc.KEPT_UIDS[0], keep=True)
    _drain(e, net)
    assert e.held() == 1
    reused = e.continue_search(dc.KEPT_UIDS[0], dc.KEPT_MOVES, sims=dc.KEPT_SIMS[1], id=dc.KEPT_UIDS[1])
    got = _drain(e, net)[dc.KEPT_UIDS[1]]
    an.close()
    assert reused == n_before > 0 and got["root_n"] == n_before + dc.KEPT_SIMS[1]
    _same(got, want, dc.KEPT_SIMS[1], ("kept", history))


def test_a_slot_forgets_the_longer_window_it_held():
    """Six searches at once on two slots, the two longest windows first: every later one writes a shorter window over a longer
    one, and the entries behind its end must not count.  Each result equals the oracle's, and the same search on an engine with
    one slot that takes them shortest window first, bit for bit."""
    net = dc.shuffle_net()
    jobs = [(dc.CASES[name].position(), uid, dc.CASES[name].sims) for name, uid in dc.SLOT_JOBS]
    got = []
    for slots, order in ((2, jobs), (1, sorted(jobs, key=lambda j: len(j[0][1])))):
        an = _analyzer(net.infer_np, slots, 8, 128)
        for (fen, moves), uid, sims in order:
            an.engine.submit(fen, moves, sims=sims, id=uid)
        got.append(_drain(an.engine, net))
        an.close()
    two, one = got
    for name, uid in dc.SLOT_JOBS:
        _same(two[uid], dc.oracle_slot_job(name, uid), dc.CASES[name].sims, (name, uid))
        _equal_results(two[uid], one[uid], name)
