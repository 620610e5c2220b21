"""The draw rules a search leaf can meet beyond mate and stalemate -- the 75-move rule, fivefold repetition (the part on the
descent's own path and the part in the game's history window), insufficient material -- as cases for
tests/test_draw_rules.py (oracle alone, no GPU: every case is shown to meet its rule, and to notice when the rule is bent) and
tests/test_draw_rules_gpu.py (leaf_terminal of csrc/tree_select.hip against the oracle).

`CountingMCTS` is the oracle's MCTS (oracle/mcts_ref.py, left as it is) that tallies every terminal leaf by the first rule that
applies, in the engine's order; `MutantMCTS` replaces the game-over test by a predicate: a threshold moved by one, a rule
dropped.  Mutants that are no predicate are control inputs: the same root with a shorter history, or with none.

Out of scope: the early exit of the engine's path scan at an irreversible move (`broke`, tree_select.hip).  It cannot change a
result short of a 64-bit key collision -- an irreversible move changes a component of the position key for good (a man leaves
the board, a pawn leaves its square for ever, a castling right is lost), so no position behind it can equal one before it and
the scan would count nothing there anyway.  No case here tries to test it."""
import functools

import numpy as np

from oracle import chess_py as ch
from oracle import mcts_ref as ref
from tests import gumbel_ref as gr
from tests import proof_ref as pr
from tests.fake_net import FakeNet
from tests.hash_net import HashNet
from tests.test_analysis_gpu import MULTIPV, PV_LEN, _oracle_lines
from tests.test_search_gpu import MCTS
from tests.test_tb_search_gpu import RIGHT_LEFT, TbMCTS

SEED = 1234
KINDS = ("mate", "stalemate", "insufficient", "75", "5fold")
S = ["g1f3", "g8f6", "f3g1", "f6g8"]                         # the knights out and home: the start position again


def tour(k):
    """4 + 4 k reversible plies from the start position back to it that never pass through it on the way."""
    return ["b1c3", "b8c6"] + ["c3e4", "c6e5", "e4c3", "e5c6"] * k + ["c3b1", "c6b8"]


# ---- group 1: the 75-move rule.  Quiet moves run the clock out, pawn moves and captures reset it.
FEN75 = "8/2p5/3p4/KP5r/1R3p1k/8/4P1P1/8 w - - {} 80"
# ---- group 2: fivefold repetition, every root the start position plus moves
MOVES_2A = S * 3                                             # window of 12: the start position at 0, 4, 8
MOVES_2B = S * 2                                             # window of 8: at 0, 4
MOVES_2C = S + tour(14) + S + S[:3]                          # window of 71: at 0, 4, 64, 68
MOVES_2D = tour(15) + tour(15) + S + S[:3]                   # window of 135: at 0, 64, 128, 132
MOVES_2E = S * 50                                            # 200 plies: more than the engine's window holds
MOVES_KEPT = S * 2 + S[:2]                                   # the kept tree: continued by f3g1 f6g8 it is 2a's root
# ---- group 3
KBKN = "8/8/8/3k4/8/2n5/1B6/K7 w - - 0 1"
# ---- group 4: every child a 3-man table win and a 75-move draw
TB_149 = RIGHT_LEFT.replace(" 0 1", " 149 90")


def fake_net():
    return FakeNet(seed=3, sharp=0.5)


def shuffle_net():
    """A flat hash evaluator that favours the four moves of S, each for its own side."""
    b = ch.Board(ch.START_FEN)
    idx = []
    for u in S:
        m = ch.Move.from_uci(u)
        idx.append(ch.move_to_index(b, m))
        b.push(m)
    return HashNet(seed=41, sharp=2.0, vscale=0.3, boost_white=[(idx[0], 6.0), (idx[2], 6.0)],
                   boost_black=[(idx[1], 6.0), (idx[3], 6.0)])


class Case:
    def __init__(self, name, fen, moves, net, sims, uid):
        self.name, self.fen, self.moves, self.net, self.sims, self.uid = name, fen, list(moves), net, sims, uid

    def root_fen(self, keep=None):
        """The FEN the history starts from; keep = n: only the last n moves are history, the others are folded into the FEN
        (0: the bare FEN of the root)."""
        b = ch.Board(self.fen)
        for u in (self.moves if keep is None else self.moves[: len(self.moves) - keep]):
            b.push(ch.Move.from_uci(u))
        return self.fen if keep is None else b.fen()

    def position(self, keep=None):
        """What the analysis engine is given: (fen, moves)."""
        return self.root_fen(keep), (self.moves if keep is None else self.moves[len(self.moves) - keep:])


CASES = {c.name: c for c in [
    Case("1a", FEN75.format(147), [], fake_net, 64, 7),
    Case("1b", FEN75.format(148), [], fake_net, 64, 7),
    Case("1c", FEN75.format(149), [], fake_net, 64, 7),
    Case("2a", ch.START_FEN, MOVES_2A, shuffle_net, 128, 9),
    Case("2b", ch.START_FEN, MOVES_2B, shuffle_net, 128, 9),
    Case("2c", ch.START_FEN, MOVES_2C, fake_net, 128, 9),
    Case("2d", ch.START_FEN, MOVES_2D, fake_net, 128, 9),
    Case("3a", KBKN, [], fake_net, 64, 11),
]}


def replay(fen, moves):
    """The board after `moves`, and the repetition window as the engine's host keeps it (host_rules.h, RepWindow): the keys of
    the positions before each trailing reversible move.  Every move is asserted legal; the second value lists, per move,
    whether it was reversible (no capture, no pawn move, no castling right lost)."""
    b = ch.Board(fen)
    window, reversible = [], []

    def rights(bb):
        return tuple(f(c) for c in (True, False) for f in (bb.has_kingside_castling_rights, bb.has_queenside_castling_rights))

    for u in moves:
        m = ch.Move.from_uci(u)
        assert b.is_legal(m), (u, b.fen())
        key, clock, before = b._transposition_key(), b.halfmove_clock, rights(b)
        b.push(m)
        rev = b.halfmove_clock == clock + 1 and rights(b) == before
        reversible.append(rev)
        window = window + [key] if rev else []
    return b, window, reversible


# ---- the oracle that counts, and the mutants
class Counting:
    """Mix-in ahead of an oracle MCTS class: terminal leaves by kind, the first rule of the engine's order that applies."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.kinds = {k: 0 for k in KINDS}
        self.sims_asked = 0

    @staticmethod
    def kind_of(leaf):
        if leaf.is_checkmate():
            return "mate"
        if leaf.is_stalemate():
            return "stalemate"
        if leaf.is_insufficient_material():
            return "insufficient"
        if leaf.is_seventyfive_moves():
            return "75"
        if leaf.is_fivefold_repetition():
            return "5fold"
        return None

    def terminal_value(self, leaf):
        k = self.kind_of(leaf)
        if k is not None:
            self.kinds[k] += 1
        return super().terminal_value(leaf)

    def run_batched(self, board, root, sims):
        self.sims_asked += sims
        return super().run_batched(board, root, sims)

    @property
    def terminal_leaves(self):
        return sum(self.kinds.values())

    @property
    def network_leaves(self):
        """Simulations that ended in an evaluation (a table hit is neither)."""
        return self.sims_asked - self.terminal_leaves - getattr(self, "tb_leaves", 0)


class CountingMCTS(Counting, ref.MCTS):
    pass


class CountingTbMCTS(Counting, TbMCTS):
    pass


class CountingProofMCTS(Counting, pr.ProofMCTS):
    pass


def over_with(seventyfive=150, fold=5):
    """The game-over test with its two numbers open: None drops the rule.  (150, 5) is Board.is_game_over()."""
    def over(b):
        if b.is_checkmate() or b.is_stalemate() or b.is_insufficient_material():
            return True
        if seventyfive is not None and b.halfmove_clock >= seventyfive:
            return True
        return fold is not None and b.is_repetition(fold)
    return over


MUTANTS_75 = {"75 at 149": over_with(seventyfive=149), "75 at 151": over_with(seventyfive=151), "75 dropped": over_with(seventyfive=None)}
MUTANTS_5FOLD = {"fold at 4": over_with(fold=4), "fold at 6": over_with(fold=6), "fold dropped": over_with(fold=None)}
PREDICATES = {**MUTANTS_75, **MUTANTS_5FOLD, "true rules": over_with()}      # the last one: the harness checked against itself


class MutantMCTS(ref.MCTS):
    """The oracle with `over(leaf)` in place of leaf.is_game_over(); a leaf that is over and no mate is a draw.  `ended` counts
    the leaves the predicate ended."""

    def __init__(self, *a, over, **kw):
        super().__init__(*a, **kw)
        self.over, self.ended = over, 0

    def terminal_value(self, leaf):
        return -1.0 if leaf.is_checkmate() else float(self.cfg.draw_penalty)

    def run_batched(self, board, root, sims):
        L = int(self.cfg.inference_batch_size) or 96
        done = 0
        while done < sims:
            batch_n = min(L, sims - done)
            inflight = {} if self.cfg.virtual_loss_active else None
            samples = []
            for _ in range(batch_n):
                node, path, leaf = self.select(board.copy(), root, inflight)
                if self.over(leaf):
                    self.ended += 1
                    self.backpropagate(path, self.terminal_value(leaf))
                else:
                    samples.append((node, list(path), leaf))
            if samples:
                x = np.stack([ch.encode_board(b) for (_, _, b) in samples], axis=0)
                pol, val = self.infer_np(x)
                self.evals += len(samples)
                for (node, path, leaf), p, v in zip(samples, pol, val):
                    if not node.expanded:
                        self.expand(node, leaf, p)
                        self.register_children(node, leaf)
                    self.backpropagate(path, float(np.clip(v, -1.0, 1.0)))
            done += batch_n


def oracle_cfg(L=8, vl=True, use_tt=False):
    return ref.MCTSConfig.from_dict(dict(MCTS, inference_batch_size=L, use_tt=use_tt, virtual_loss_active=vl, dirichlet_plies=0,
                                         numerics="engine"))


def expectation(o, board, root, rq):
    """An oracle search as tests/test_analysis_gpu._check reads it, with all root visit counts and the oracle itself."""
    return {"status": "ok", "lines": _oracle_lines(root, MULTIPV, PV_LEN), "evals": o.evals, "root_n": root.n, "root_q": rq,
            "nlegal": len(board.legal_moves), "counts": [c.n for c in root.children.values()],
            "idx": [c.move_idx for c in root.children.values()], "oracle": o}


@functools.lru_cache(maxsize=None)
def oracle_run(name, L=8, vl=True, use_tt=False, keep=None, mutant=None, net=None, uid=None):
    """The oracle's search of a case (computed once per argument set, never modified).  `mutant`: a key of PREDICATES;
    `keep`: see Case.root_fen; `net`, `uid`: another evaluator (a function of this module) and game id than the case's own."""
    case = CASES[name]
    fen, moves = case.position(keep)
    board = ch.Board(fen)
    for u in moves:
        board.push(ch.Move.from_uci(u))
    cfg = oracle_cfg(L, vl, use_tt)
    infer, game = (net or case.net)().infer_np, case.uid if uid is None else uid
    if mutant is None:
        o = CountingMCTS(cfg, infer, seed=SEED, game=game)
    else:
        o = MutantMCTS(cfg, infer, seed=SEED, game=game, over=PREDICATES[mutant])
    assert not board.is_game_over(), name
    _, _, rq = o.run(board, num_simulations=case.sims, ply=0)
    return expectation(o, board, o._last_root, rq)


# ---- slots: all of these at once on an engine with two slots, one evaluator (shuffle_net) for all, ids of their own.  The two
# long windows take the slots first; every later search then writes a shorter window over a longer one.
SLOT_JOBS = [("2c", 31), ("2d", 32), ("2a", 33), ("1c", 34), ("3a", 35), ("2b", 36)]
SLOT_RULE = {"2c": "5fold", "2d": "5fold", "2a": "5fold", "2b": "5fold", "1c": "75", "3a": "insufficient"}


def oracle_slot_job(name, uid):
    return oracle_run(name, net=shuffle_net, uid=uid)


def kinds_line(tag, want):
    o = want["oracle"]
    return f"{tag}: {o.kinds}, {o.network_leaves} network leaves, {o.evals} evaluations"


@functools.lru_cache(maxsize=None)
def oracle_tb(fen, L=8, vl=True, uid=77):
    """Group 4: the oracle with the reference generator's 3-man tables, on the evaluator of tests/test_tb_search_gpu.py."""
    from tests import tb_util as tu
    o = CountingTbMCTS(oracle_cfg(L, vl), FakeNet(seed=3, sharp=8.0).infer_np, seed=SEED, game=uid, tables=tu.ref_tables())
    _, _, rq = o.run(ch.Board(fen), num_simulations=64, ply=0)
    return o, rq


PROOF_UID = {"1c": 9, "2a": 9}              # 1c: no children scan of the reference is decided by less than 1e-4


@functools.lru_cache(maxsize=None)
def oracle_proof(name, L, vl=True):
    """Group 5: the reference of the proof search (tests/proof_ref.py) on a case: (oracle, its result)."""
    case = CASES[name]
    board, _, _ = replay(case.fen, case.moves)
    o = CountingProofMCTS(oracle_cfg(L, vl), case.net().infer_np, seed=SEED, game=PROOF_UID[name])
    return o, o.search(board, case.sims)


# ---- modes that only the split-step search of a self-play engine has (the position table, the Gumbel root): it takes a FEN and
# no moves, so the history is played in -- a search of one simulation per ply, then search_advance with the scripted move.  The
# oracle does the same, search by search, so both sides have drawn the same numbers from the game's streams when the search that
# counts begins.
class CountingGumbelMCTS(Counting, gr.GumbelMCTS):
    pass


def _fresh_counts(o):
    o.kinds = {k: 0 for k in KINDS}
    o.sims_asked, o.evals = 0, 0


@functools.lru_cache(maxsize=None)
def oracle_played_tt(name, L=8, vl=True):
    """A case with the position table on (use_tt; the engine's compat.tt_merge, whose table lives for one search)."""
    case = CASES[name]
    o = CountingMCTS(oracle_cfg(L, vl, use_tt=True), case.net().infer_np, seed=SEED, game=case.uid)
    board = ch.Board(case.fen)
    for u in case.moves:
        if board.is_game_over():
            # a position of the tour for the fifth time or more: run() answers without a search, the engine searches what it
            # is given -- the steps of run() behind its test (as tests/test_analysis_gpu._oracle_run), which draw what it draws
            root = ref.Node()
            logits, _ = o._infer_one(board)
            o.expand(root, board, logits, is_root=True)
            o.run_batched(board, root, 1)
        else:
            o.run(board, num_simulations=1, ply=0)
        o.tt.clear()
        o.nn_cache.clear()
        board.push(ch.Move.from_uci(u))
    _fresh_counts(o)
    assert not board.is_game_over(), name
    _, _, rq = o.run(board, num_simulations=case.sims, ply=0)
    return expectation(o, board, o._last_root, rq)


@functools.lru_cache(maxsize=None)
def oracle_played_gumbel(name, L=8, vl=True):
    """A case under the Gumbel root search (tests/gumbel_ref.py, its defaults): (oracle, result of its last search, root FEN)."""
    case = CASES[name]
    o = CountingGumbelMCTS(oracle_cfg(L, vl), case.net().infer_np, seed=SEED, game=case.uid, **gr.DEFAULTS)
    board = ch.Board(case.fen)
    for u in case.moves:
        assert not board.is_game_over(), name                # (a root that is over would need the steps of search() by hand)
        o.search(board, 1)
        board.push(ch.Move.from_uci(u))
    _fresh_counts(o)
    o.rows = []
    assert not board.is_game_over(), name
    return o, o.search(board, case.sims), board.fen()


# ---- the kept tree: a search with keep, continued behind two moves on its own subtree
KEPT_UIDS, KEPT_SIMS, KEPT_MOVES = (20, 21), (64, 128), S[2:]


@functools.lru_cache(maxsize=None)
def oracle_kept(history):
    """MCTS.run on the subtree behind KEPT_MOVES of a searched root, as tests/test_analysis_live_gpu._oracle_continue grafts it
    (that helper builds its board from a FEN alone and fixes evaluator and budget, so its few lines are restated here with the
    moves that led to the root): (visits of the kept node before, expectation).  history False: both searches know the root
    of the first one only as a bare FEN."""
    first, _, _ = replay(ch.START_FEN, MOVES_KEPT)
    board = first if history else ch.Board(first.fen())
    o1 = ref.MCTS(oracle_cfg(), shuffle_net().infer_np, seed=SEED, game=KEPT_UIDS[0])
    o1.run(board, num_simulations=KEPT_SIMS[0], ply=0)
    parent, node = None, o1._last_root
    for u in KEPT_MOVES:
        last = ch.Move.from_uci(u)
        parent, node = node, node.children[last]
        board.push(last)
    n_before = node.n
    o = CountingMCTS(oracle_cfg(), shuffle_net().infer_np, seed=SEED, game=KEPT_UIDS[1])
    o._last_root, o._last_move = parent, last
    _, _, rq = o.run(board, num_simulations=KEPT_SIMS[1], ply=0)
    assert o._last_root is node
    return n_before, expectation(o, board, node, rq)
