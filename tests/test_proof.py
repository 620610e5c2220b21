"""The proof search without a GPU: the host export of csrc/proof_core.h (m0_proof_combine) against the rule written out in
tests/proof_ref.py, that file's reference search against its exhaustive minimax, and the pieces of the Python side that need no
engine."""
import ctypes as C
import itertools

import numpy as np
import pytest

from matrix0_amd import _lib, engine as eng
from oracle import chess_py as ch
from oracle import mcts_ref as ref
from tests import proof_ref as pr
from tests.fake_net import FakeNet
from tests.test_search_gpu import MCTS

STATES = [pr.NONE, pr.WIN, pr.LOSS, pr.DRAW]


def _children(k):
    """Every list of k children: a state each, plies 0..3 for a win or a loss, 0 otherwise."""
    one = [(s, p) for s in STATES for p in (range(4) if s in (pr.WIN, pr.LOSS) else [0])]
    return itertools.product(one, repeat=k)


def test_combine_equals_the_rule_for_every_small_family():
    assert eng.PROOF_STATES == STATES
    n = 0
    for k in (1, 2, 3):
        for kids in _children(k):
            for complete in (False, True):
                got = eng.proof_combine([s for s, _ in kids], [p for _, p in kids], complete)
                assert got == pr.combine(list(kids), complete), (kids, complete, got)
                n += 1
    assert n == 2 * (10 + 10 ** 2 + 10 ** 3)


def test_combine_over_a_wide_node_takes_the_extremes():
    states, plies = [pr.WIN] * 256, list(range(256))
    assert eng.proof_combine(states, plies, True) == (pr.LOSS, 256)
    assert eng.proof_combine(states, plies, False) == (pr.NONE, 0)
    states[200], states[17] = pr.LOSS, pr.LOSS
    assert eng.proof_combine(states, plies, False) == (pr.WIN, 18)
    assert eng.proof_combine([pr.WIN] * 255 + [pr.DRAW], [5] * 255 + [0], True) == (pr.DRAW, 0)
    assert eng.proof_combine([pr.WIN] * 255 + [pr.NONE], [5] * 255 + [0], True) == (pr.NONE, 0)


def test_combine_refuses_what_it_cannot_read():
    L = _lib.lib()
    one = np.zeros(1, np.int32)
    st, pl = C.c_int(7), C.c_int(7)
    assert L.m0_proof_combine(1, _lib.ptr(one), _lib.ptr(one), 1, None, None) == _lib.M0_OK
    assert L.m0_proof_combine(0, _lib.ptr(one), _lib.ptr(one), 1, C.byref(st), C.byref(pl)) == _lib.M0_ERR_INVALID
    assert L.m0_proof_combine(257, _lib.ptr(one), _lib.ptr(one), 1, C.byref(st), C.byref(pl)) == _lib.M0_ERR_INVALID
    assert L.m0_proof_combine(1, None, _lib.ptr(one), 1, C.byref(st), C.byref(pl)) == _lib.M0_ERR_INVALID
    for bad_state, bad_plies in [(4, 0), (-1, 0), (1, -1), (1, 8192)]:
        s, p = np.array([bad_state], np.int32), np.array([bad_plies], np.int32)
        assert L.m0_proof_combine(1, _lib.ptr(s), _lib.ptr(p), 1, C.byref(st), C.byref(pl)) == _lib.M0_ERR_INVALID
    with pytest.raises(ValueError):
        eng.proof_combine([pr.WIN, pr.WIN], [1], True)


def test_the_minimax_solves_the_positions_as_listed():
    for fen, state, plies, nlegal in pr.POSITIONS:
        assert len(list(ch.Board(fen).legal_moves)) == nlegal, fen
        assert pr.solve(fen, 4) == (state, plies), fen
        if plies > 0:
            assert pr.solve(fen, plies - 1) == (pr.NONE, 0), fen


def _check_against_minimax(fen, o, want):
    """Every state the search reports is the minimax value; a distance is an upper bound of the shortest one."""
    board = ch.Board(fen)
    for node, (state, plies) in [(want["root"], (want["state"], want["plies"]))] + \
            list(zip(want["root"].children.values(), want["children"])):
        if state == pr.NONE:
            continue
        b = board.copy()
        if node is not want["root"]:
            b.push(node.move)
        true_state, true_plies = pr.solve(b.fen(), max(plies, 3))
        assert true_state == state and true_plies <= plies, (fen, node.move, (state, plies), (true_state, true_plies))


@pytest.mark.parametrize("L", [1, 4, 16])
def test_the_reference_search_reports_minimax_values(L):
    for j, (fen, state, plies, _) in enumerate(pr.POSITIONS):
        cfg = ref.MCTSConfig.from_dict(dict(MCTS, inference_batch_size=L, use_tt=False, virtual_loss_active=True,
                                            numerics="engine"))
        o = pr.ProofMCTS(cfg, FakeNet(seed=3, sharp=8.0).infer_np, seed=1234, game=100 + j)
        want = o.search(ch.Board(fen), 200)
        _check_against_minimax(fen, o, want)
        if want["state"] != pr.NONE:
            assert want["state"] == state and want["plies"] >= plies, fen
            assert o.sims < 200 or L > 1, "a search whose root is proven ends"
            kids = want["children"]
            assert 0 <= want["pick"] < len(kids)
            if state == pr.WIN:
                assert kids[want["pick"]] == (pr.LOSS, want["plies"] - 1)
        # a proven node is never walked through: nothing below it was visited after the proof, and every proven node's
        # children block is consistent with the rule
        for node, got in o.proofs.items():
            if node.children:
                assert got == pr.combine([o.proof(c) for c in node.children.values()], True) or got[0] == pr.WIN


def test_pruned_children_prove_wins_only():
    fen = pr.POSITIONS[3][0]                 # one legal move, lost: with pruning the children are not known to be all moves
    cfg = ref.MCTSConfig.from_dict(dict(MCTS, inference_batch_size=4, use_tt=False, virtual_loss_active=True, numerics="engine",
                                        max_children=8))
    o = pr.ProofMCTS(cfg, FakeNet(seed=3, sharp=8.0).infer_np, seed=1234, game=7)
    want = o.search(ch.Board(fen), 64)
    assert want["state"] == pr.NONE and o.sims == 64
    assert all(s in (pr.WIN, pr.NONE) or not n.children for n, (s, _) in o.proofs.items())


def test_pick_follows_the_table():
    W, Lo, D, N = pr.WIN, pr.LOSS, pr.DRAW, pr.NONE
    assert pr.pick(W, [(N, 0), (Lo, 4), (Lo, 2), (Lo, 2)], [9, 1, 1, 5]) == 2
    assert pr.pick(Lo, [(W, 3), (W, 5), (W, 5)], [9, 1, 1]) == 1
    assert pr.pick(D, [(W, 3), (D, 0), (D, 0)], [9, 2, 7]) == 2
    assert pr.pick(N, [(W, 3), (N, 0), (D, 0)], [9, 4, 4]) == 1
    assert pr.pick(N, [(W, 3), (W, 1)], [2, 9]) == 1


# ---- the UCI side: the option ProveMates, `score mate` for proven lines, `go mate` (no engine behind it: tests/test_uci.py's fake)
from matrix0_amd import uci                                  # noqa: E402
from tests import test_uci as tu                             # noqa: E402


class _ProvingEngine(tu._FakeEngine):
    """The fake one-slot engine of tests/test_uci.py in the proof search: from its `proven_after`-th step on its results say
    that the best line mates in `plies` plies, and a search whose root is proven ends by itself when `ends` is set."""

    def __init__(self, proven_after=3, plies=3, ends=True, **kw):
        super().__init__(**kw)
        self.proven_after, self.plies, self.ends = proven_after, plies, ends

    def _result(self):
        r = super()._result()
        proven = self.run["steps"] >= self.proven_after and r["lines"]
        r["proof"], r["proof_plies"] = ("win", self.plies) if proven else ("none", 0)
        for k, ln in enumerate(r["lines"]):
            ln["proof"], ln["proof_plies"] = ("win", self.plies) if proven and k == 0 else (("loss", 4) if proven else ("none", 0))
        return r

    def step(self, steps=1):
        super().step(steps)
        if self.ends and self.run is not None and self.run["steps"] >= self.proven_after:
            self.done.append(self._result())
            self._finish()


def test_prove_mates_is_off_by_default_and_go_mate_is_then_ignored():
    u, e, out, _ = tu._uci(_ProvingEngine())
    assert u.unlisted["ProveMates"] is False
    u.command("uci")
    assert not any("ProveMates" in o for o in out) and len([o for o in out if o.startswith("option name ")]) == 6
    u.command("go mate 2 nodes 64")
    assert "info string go mate is not supported and ignored" in out
    tu._drive(u)
    # an engine that reports proofs all the same: the scores stay centipawns unless the option is on?  No: a proof is a proof,
    # whoever asked for it -- but nothing ends the search for `mate`
    assert u.search is None and u.__dict__["held"] is not None


def test_prove_mates_parsing():
    u, e, out, _ = tu._uci(_ProvingEngine())
    for value, word in (("maybe", "needs true or false"), ("", "needs true or false"), ("1", "needs true or false")):
        u.command(f"setoption name ProveMates value {value}")
        assert word in out[-1] and u.unlisted["ProveMates"] is False
    u.command("setoption name provemates value TRUE")
    assert u.unlisted["ProveMates"] is True and u.dirty            # the mode is set before an engine's first search: a new engine
    u.command("setoption name ProveMates value false")
    assert u.unlisted["ProveMates"] is False
    assert uci.parse_go("mate 3".split()) == ({"mate": 3}, []) and uci.parse_go(["mate"]) == ({}, ["mate"])
    assert uci.build_parser().parse_args(["--config", "c", "--checkpoint", "k", "--prove"]).prove is True
    from matrix0_amd import analysis
    assert analysis.build_parser().parse_args(["--config", "c", "--checkpoint", "k", "--fens", "f", "--prove"]).prove is True


def test_go_mate_is_honoured_and_proven_lines_print_score_mate():
    rebuilt = []

    def rebuild(options):
        rebuilt.append(dict(options))
        e2 = _ProvingEngine(proven_after=3, plies=3, ends=False)
        return e2, (lambda: e2.step(1))

    u, e, out, _ = tu._uci(_ProvingEngine(), rebuild=rebuild)
    u.command("setoption name ProveMates value true")
    u.command("setoption name MultiPV value 2")
    u.command("go mate 2 depth 5")
    assert rebuilt and rebuilt[0]["ProveMates"] is True and e.closed
    assert [o for o in out if "ignored" in o] == ["info string go depth is not supported and ignored"]
    assert u.search["mate"] == 2
    e2 = u.engine
    while u.pump():
        pass
    # ended by the mate it asked for, long before MaxNodes (256 simulations = 33 steps of this engine)
    assert [x[0] for x in e2.log].count("step") <= 5 and ("stop", 1) in e2.log
    infos = [o for o in out if o.startswith("info depth")]
    assert any(" multipv 1 score mate 2 " in o for o in infos) and any(" multipv 2 score mate -2 " in o for o in infos)
    assert out[-1].startswith("bestmove e2e4")
    # a mate that is too far for `go mate 1` does not end the search: its other limits do
    out.clear()
    u.command("ucinewgame")
    u.command("go mate 1 nodes 64")
    n = len(e2.log)
    while u.pump():
        pass
    assert [x[0] for x in e2.log[n:]].count("step") == 64 // 8 + 1 and not any(x[0] == "stop" for x in e2.log[n:])
    assert any(" score mate 2 " in o for o in out)


def test_mate_score_of_proven_distances():
    assert [uci.mate_score(p, False) for p in (1, 3, 5)] == [1, 2, 3]
    assert [uci.mate_score(p, True) for p in (2, 4)] == [-1, -2]
