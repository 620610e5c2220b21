"""Reference of the self-play budget mix (include/m0_budget.h) in Python and numpy: the full-or-fast draw, the forced-playout
threshold, the pruning of a root's visits into a policy target, a search that applies the deficit rule at depth 0 of the oracle's
MCTS (oracle/mcts_ref.py, imported and left as it is) with the engine's random streams, and a short self-play loop over the
oracle's decision functions.

The search and the pruning record the smallest margins of their decisions: the smallest |n + f - sqrt(k P N)| / sqrt(k P N) of
any deficit test and the smallest |PUCT(i; m) - S| of any pruning test.  Parity with an engine whose statistics differ in the
last bits only means something where no decision was that close; the tests assert MIN_DEFICIT_MARGIN and MIN_PRUNE_MARGIN
before they compare."""
import math

import numpy as np

from oracle import chess_py as ch
from oracle import mcts_ref as ref

PURPOSE_BUDGET = 7            # csrc/budget_core.h
DEFAULTS = {"full_prob": 0.25, "fast_simulations": 100, "forced_k": 2.0, "prune_targets": True}
MIN_DEFICIT_MARGIN = 1e-9
MIN_PRUNE_MARGIN = 1e-7


def is_full(seed, game, ply, full_prob):
    """full = u < full_prob with u the draw `ply` of the stream of (seed, game, PURPOSE_BUDGET)"""
    return ref.Stream(ref.derive_seed(seed, game, PURPOSE_BUDGET)).at(ply) < full_prob


def n_forced(forced_k, prior, n_sum):
    return math.sqrt(forced_k * prior * float(n_sum))


def puct(q, c, p, sq, m):
    return q + c * p * sq / (1.0 + float(m))


def prune(prior, q, n, root_n, cpuct, forced_k):
    """(pruned_n, pi, best, margin): margin = the smallest |PUCT(i; m) - S| of the tests made (inf: none)."""
    k = len(n)
    n = [int(x) for x in n]
    margin = math.inf
    best = -1
    for i in range(k):
        if n[i] > 0 and (best < 0 or n[i] > n[best]):
            best = i
    m = list(n)
    total = sum(n)
    if best >= 0:
        sq = math.sqrt(float(max(1, int(root_n))))
        S = puct(float(q[best]), cpuct, float(prior[best]), sq, n[best])
        for i in range(k):
            if i == best or n[i] <= 0:
                continue
            F = min(float(n[i]), math.ceil(n_forced(forced_k, float(prior[i]), total)))
            F = int(F)
            mi = n[i]
            for c in range(n[i] - F, n[i] + 1):
                v = puct(float(q[i]), cpuct, float(prior[i]), sq, c)
                margin = min(margin, abs(v - S))
                if v < S:
                    mi = c
                    break
            if mi == 1 and n[i] > 1:
                mi = 0
            m[i] = mi
    sm = sum(m)
    pi = np.array([x / sm if sm > 0 else 0.0 for x in m], np.float64)
    return np.array(m, np.int32), pi, best, margin


class BudgetMCTS(ref.MCTS):
    """oracle.mcts_ref.MCTS with the mode's two switches per search: `forced_k` > 0 applies the deficit rule at depth 0 of
    select, `fast` turns the Dirichlet noise off."""

    def __init__(self, cfg, infer, seed=1234, game=0):
        super().__init__(cfg, infer, seed=seed, game=game)
        self.forced_k = 0.0               # of the running search: 0 = a search without the rule
        self.fast = False
        self.forced_descents = 0
        self.min_deficit_margin = math.inf
        self.rows = []                    # network rows of every pass, a root's own evaluation included

    def add_dirichlet(self, root):
        if not self.fast:
            super().add_dirichlet(root)

    def _infer_one(self, board):
        self.rows.append(1)
        return super()._infer_one(board)

    def _deficit_child(self, root, inflight):
        """the lowest root child in deficit, or None"""
        kids = list(root.children.values())
        n_sum = sum(c.n for c in kids)
        found = None
        for c in kids:
            if c.n <= 0:
                continue
            f = inflight.get(c, 0) if inflight is not None else 0
            thr = n_forced(self.forced_k, float(c.prior), n_sum)
            if thr > 0.0:
                self.min_deficit_margin = min(self.min_deficit_margin, abs(float(c.n + f) - thr) / thr)
            if found is None and float(c.n + f) < thr:
                found = c
        return found

    def select(self, board, root, inflight):
        """MCTS.select, line by line, with the deficit rule at depth 0: the jitter draws of the root's children are consumed
        whichever rule decides."""
        cfg = self.cfg
        node = root
        path = [root]
        while node.expanded:
            if not node.children:
                break
            parent_visits = max(1, node.n)
            best_score, best = -1e9, None
            eff = self.cpuct_at(max(0, len(path) - 1))
            for child in node.children.values():
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
                if score > best_score:
                    best_score, best = score, child
            if node is root and self.forced_k > 0.0:
                forced = self._deficit_child(root, inflight)
                if forced is not None:
                    best = forced
                    self.forced_descents += 1
            board.push(best.move)
            node = best
            path.append(node)
            if inflight is not None:
                inflight[best] = inflight.get(best, 0) + 1
        return node, path, board

    def run_batched(self, board, root, sims):
        """MCTS.run_batched (tree-only), recording the rows of every pass."""
        assert not self.cfg.use_tt
        L = int(self.cfg.inference_batch_size) or 96
        done = 0
        while done < sims:
            batch_n = min(L, sims - done)
            self._pass += 1
            inflight = {} if self.cfg.virtual_loss_active else None
            samples = []
            for _ in range(batch_n):
                node, path, leaf = self.select(board.copy(), root, inflight)
                if leaf.is_game_over():
                    self.backpropagate(path, self.terminal_value(leaf))
                else:
                    samples.append((node, list(path), leaf))
            self.rows.append(len(samples))
            if samples:
                x = np.stack([ch.encode_board(b) for (_, _, b) in samples], axis=0)
                pol, val = self.infer_np(x)
                self.evals += len(samples)
                for (node, path, leaf), p, v in zip(samples, pol, val):
                    if not node.expanded:
                        self.expand(node, leaf, p)
                    self.backpropagate(path, float(np.clip(v, -1.0, 1.0)))
            done += batch_n

    def search(self, board, sims, ply=0, forced_k=0.0, fast=False):
        """MCTS.run for one search of the mode: the root's children afterwards."""
        self.forced_k, self.fast = (0.0 if fast else float(forced_k)), bool(fast)
        self.run(board, num_simulations=sims, ply=ply)
        return list(self._last_root.children.values())


def play_game(cfg_dict, infer_np, seed, game_uid, budget, virtual_loss_active=True):
    """One self-play game of an engine in the mode, with the subtree of the played move kept: the loop of
    oracle/selfplay_ref.play_game without book and opening plies, over the same helpers.  `budget`: the four values of
    m0_budget_cfg.  Returns moves, full, sims, pi per ply, z, and the margins of all its searches and prunings."""
    from oracle import selfplay_ref as sr
    sp = cfg_dict.get("selfplay", {}) or {}
    draw_cfg = sr.draw_cfg_of(cfg_dict)
    mcfg = sr.mcts_config_for_worker(cfg_dict, False, use_tt=False, virtual_loss_active=virtual_loss_active, numerics="engine")
    mcts = BudgetMCTS(mcfg, infer_np, seed=seed, game=game_uid)
    game = ref.Stream(ref.derive_seed(seed, game_uid, ref.PURPOSE_GAME))
    board = ch.Board()
    history = []
    temp_start, temp_end = float(sp.get("temperature_start", 1.0)), float(sp.get("temperature_end", 0.1))
    temp_moves, window_k = int(sp.get("temperature_moves", 20)), int(sp.get("resign_window", 4))
    max_len = int(sp.get("max_game_len", 200))
    st = ref.ResignState()
    pis, fulls, sims_used, turns, values = [], [], [], [], []
    prune_margin = math.inf
    z = None
    while not board.is_game_over() and len(pis) < max_len:
        if ref.should_adjudicate_draw(board, history, draw_cfg):
            break
        ply = len(pis)
        temperature = ref.temperature_for(board.fullmove_number, temp_start, temp_end, temp_moves)
        full = is_full(seed, game_uid, ply, budget["full_prob"])
        sims = mcfg.num_simulations if full else int(budget["fast_simulations"])
        if mcfg.playout_random_frac > 0 and mcfg.num_simulations > 0:
            sims = ref.playout_cap(sims, mcfg.playout_random_frac, game.next())
        kids = mcts.search(board, sims, ply=ply, forced_k=budget["forced_k"], fast=not full)
        root = mcts._last_root
        visits = [c.n for c in kids]
        assert sum(visits) > 0
        target = np.array(visits, np.float64) / float(sum(visits))
        if full and budget["prune_targets"] and budget["forced_k"] > 0.0:
            visits, target, _, margin = prune([c.prior for c in kids], [c.q for c in kids], visits, root.n, mcts.cpuct_at(0),
                                              budget["forced_k"])
            visits = [int(x) for x in visits]
            prune_margin = min(prune_margin, margin)
        pi = np.zeros(4672, np.float32)
        pi[[c.move_idx for c in kids]] = target
        v = float(root.q)
        k = ref.sample_move_index(visits, temperature, game.next() if ref.sample_move_draws(visits, temperature) else 0.0)
        st.recent_entropies.append(ref.policy_entropy(pi))
        if len(st.recent_entropies) > window_k:
            st.recent_entropies.pop(0)
        pis.append(pi); fulls.append(full); sims_used.append(sims); values.append(v)
        turns.append(1 if board.turn else -1)
        if ref.resign_update(st, v, len(pis), sp):
            z = -1.0 if board.turn else 1.0
            break
        history.append(kids[k].move)
        board.push(kids[k].move)
        mcts.note_move_played(kids[k].move)
    if z is None:
        z = ref.game_result(board) if board.is_game_over(claim_draw=True) else (values[-1] if values else 0.0)
    return {"played": [m.uci() for m in history], "full": fulls, "sims": sims_used, "pi": np.array(pis, np.float32),
            "z": np.array([z * t for t in turns], np.float32), "deficit_margin": mcts.min_deficit_margin,
            "prune_margin": prune_margin, "forced_descents": mcts.forced_descents}
