"""Reference of the proof search (include/m0_proof.h) in Python: the rule that combines the children's proofs, a search that
applies it inside the oracle's MCTS (oracle/mcts_ref.py, imported and left as it is) with the engine's random streams, and an
exhaustive minimax with the oracle's rules that says what a position really is.

The search records the smallest gap between the best and the second-best score of every children scan it takes: parity of
whole trees against the engine only means something where no decision was that close."""
import math

import numpy as np

from oracle import chess_py as ch
from oracle import mcts_ref as ref

NONE, WIN, LOSS, DRAW = "none", "win", "loss", "draw"

# The positions of the tests, solved by `solve` below: (FEN, state of the side to move, plies, legal moves)
POSITIONS = [
    ("6k1/5ppp/8/8/8/8/8/R6K w - - 0 1", WIN, 1, 16),
    ("7k/8/8/8/8/8/R7/1R5K w - - 0 1", WIN, 3, 30),
    ("k7/8/1K6/8/8/8/8/QQQQQQ2 w - - 0 1", WIN, 1, 89),          # the wide node
    ("7k/R7/8/8/8/8/8/1R5K b - - 0 1", LOSS, 2, 1),
    ("1k6/8/1K6/8/8/8/8/7R b - - 0 1", LOSS, 4, 2),              # needs every child proven
    ("K7/1q6/8/8/8/8/8/7k w - - 0 1", DRAW, 0, 1),               # the only move captures into K v K
]


def combine(children, complete):
    """(state, plies) of a parent from its children's [(state, plies)]; `complete`: they are all of its legal moves."""
    lost = [p for s, p in children if s == LOSS]
    if lost:
        return WIN, 1 + min(lost)
    if complete and children and all(s != NONE for s, _ in children):
        if any(s == DRAW for s, _ in children):
            return DRAW, 0
        return LOSS, 1 + max(p for _, p in children)
    return NONE, 0


def leaf_proof(board):
    """The proof of a position without a move to look at: checkmate, stalemate, insufficient material, the 75-move rule.  What
    ends a game otherwise (fivefold repetition) depends on the path and proves nothing."""
    if board.is_checkmate():
        return LOSS, 0
    if board.is_stalemate() or board.is_insufficient_material() or board.is_seventyfive_moves():
        return DRAW, 0
    return NONE, 0


def value_of(state, draw_penalty):
    return 1.0 if state == WIN else (-1.0 if state == LOSS else float(draw_penalty))


def pick(root_state, children, visits):
    """Index of the move of a root: `children` [(state, plies)] from the view of each child's side to move."""
    k = range(len(children))
    if root_state == WIN:
        cand, key = [i for i in k if children[i][0] == LOSS], lambda i: -children[i][1]
    elif root_state == LOSS:
        cand, key = list(k), lambda i: children[i][1]
    elif root_state == DRAW:
        cand, key = [i for i in k if children[i][0] == DRAW], lambda i: visits[i]
    else:
        cand, key = [i for i in k if children[i][0] != WIN] or list(k), lambda i: visits[i]
    return max(cand, key=lambda i: (key(i), -i)) if cand else -1


# ---- exhaustive minimax
def _solve(board, depth, memo):
    """(state, plies) within `depth` plies: loss at 0 plies is checkmate, draw is stalemate or insufficient material."""
    if board.is_checkmate():
        return LOSS, 0
    if board.is_stalemate() or board.is_insufficient_material():
        return DRAW, 0
    if depth <= 0:
        return NONE, 0
    key = (board._transposition_key(), depth)
    if key not in memo:
        kids = []
        for m in board.legal_moves:
            b = board.copy(stack=False)
            b.push(m)
            kids.append(_solve(b, depth - 1, memo))
        memo[key] = combine(kids, True)
    return memo[key]


def solve(fen, max_depth):
    """The value of `fen` by iterative deepening to `max_depth` plies: the first depth that decides it gives the shortest win
    and, for a loss, the longest defence against shortest wins."""
    board, memo = ch.Board(fen), {}
    for depth in range(max_depth + 1):
        state, plies = _solve(board, depth, memo)
        if state != NONE:
            return state, plies
    return NONE, 0


class ProofMCTS(ref.MCTS):
    """oracle.mcts_ref.MCTS with the proof search: `search` is MCTS.run for a fresh tree in this mode."""

    def __init__(self, cfg, infer, seed=1234, game=0):
        super().__init__(cfg, infer, seed=seed, game=game)
        self.proofs = {}                    # Node -> (state, plies), proven nodes only
        self.min_gap = math.inf
        self.rows = []                      # network rows of every pass, the root's own evaluation first
        self.sims = 0                       # simulations of the last search
        self.complete = not (cfg.max_children and cfg.max_children > 0) and not float(cfg.min_child_prior) > 0.0

    def proof(self, node):
        return self.proofs.get(node, (NONE, 0))

    def select(self, board, root, inflight):
        """MCTS.select, line by line, but: a child that is won for its own mover is passed over unless every child is (its
        jitter draw is still consumed), and the walk stops at a proven node."""
        cfg = self.cfg
        node = root
        path = [root]
        while node.expanded:
            if not node.children:
                break
            kids = list(node.children.values())
            skip_won = any(self.proof(c)[0] != WIN for c in kids)
            parent_visits = max(1, node.n)
            best_score, best, second = -1e9, None, -math.inf
            eff = self.cpuct_at(max(0, len(path) - 1))
            for child in kids:
                q = (float(node.q) - float(cfg.fpu_reduction)) if child.n == 0 else child.q
                u = eff * child.prior * (math.sqrt(parent_visits) / (1.0 + child.n))
                score = q + u
                if cfg.no_instant_backtrack and len(path) >= 2 and child.move is not None and path[-1].move is not None:
                    prev = path[-1].move
                    if child.move.from_square == prev.to_square and child.move.to_square == prev.from_square:
                        score -= 0.01
                if inflight is not None and cfg.virtual_loss > 0.0:
                    score -= float(inflight.get(child, 0)) * float(cfg.virtual_loss)
                jit = cfg.selection_jitter if cfg.selection_jitter > 0 else 0.001
                score += (self.jitter.next() - 0.5) * jit
                if skip_won and self.proof(child)[0] == WIN:
                    continue
                if score > best_score:
                    second = best_score if best is not None else second
                    best_score, best = score, child
                elif score > second:
                    second = score
            if best is None:
                best, second = kids[0], -math.inf
            if second > -math.inf:
                self.min_gap = min(self.min_gap, best_score - second)
            board.push(best.move)
            node = best
            path.append(node)
            if inflight is not None:
                inflight[best] = inflight.get(best, 0) + 1
            if self.proof(node)[0] != NONE:
                break
        return node, path, board

    def prove(self, path, proof):
        """path[-1] is proven: its ancestors are re-examined while a state changes."""
        self.proofs[path[-1]] = proof
        for parent in reversed(path[:-1]):
            got = combine([self.proof(c) for c in parent.children.values()], self.complete)
            if got[0] == NONE:
                break
            assert parent not in self.proofs, "a proven state never changes"
            self.proofs[parent] = got

    def run_batched(self, board, root, sims):
        """MCTS.run_batched with passes that end, and a search that ends, once the root is proven."""
        L = int(self.cfg.inference_batch_size) or 96
        done = 0
        while done < sims and self.proof(root)[0] == NONE:
            batch_n = min(L, sims - done)
            self._pass += 1
            inflight = {} if self.cfg.virtual_loss_active else None
            samples = []
            made = 0
            for _ in range(batch_n):
                node, path, leaf = self.select(board.copy(), root, inflight)
                made += 1
                state = self.proof(node)[0]
                if state != NONE:
                    self.backpropagate(path, value_of(state, self.cfg.draw_penalty))
                elif leaf.is_game_over():
                    self.backpropagate(path, self.terminal_value(leaf))
                    proof = leaf_proof(leaf)
                    if proof[0] != NONE:
                        self.prove(path, proof)
                else:
                    samples.append((node, list(path), leaf))
                if self.proof(root)[0] != NONE:
                    break
            self.rows.append(len(samples))
            if samples:
                x = np.stack([ch.encode_board(b) for (_, _, b) in samples], axis=0)
                pol, val = self.infer_np(x)
                self.evals += len(samples)
                for (node, path, leaf), p, v in zip(samples, pol, val):
                    if not node.expanded:
                        self.expand(node, leaf, p)
                    self.backpropagate(path, float(np.clip(v, -1.0, 1.0)))
            done += made
        self.sims = done

    def search(self, board, sims):
        """A fresh tree, no Dirichlet noise, at most `sims` simulations: {"root", "state", "plies", "children", "pick"}."""
        assert not self.cfg.use_tt and not board.is_game_over()
        self._last_root = None
        self.rows.append(1)
        self.run(board, num_simulations=sims, ply=10 ** 6)
        root = self._last_root
        kids = list(root.children.values())
        children = [self.proof(c) for c in kids]
        state, plies = self.proof(root)
        return {"root": root, "state": state, "plies": plies, "children": children,
                "pick": pick(state, children, [c.n for c in kids])}
