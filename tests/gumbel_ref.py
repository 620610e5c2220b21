"""Reference of the Gumbel root search (include/m0_gumbel.h) in Python and numpy: the considered-visits schedule of mctx's
gumbel_muzero_policy, the scores and the improved policy, and a search that applies the root rule at depth 0 of the oracle's
MCTS (oracle/mcts_ref.py, imported and left as it is) with the engine's random streams.

The search records the smallest gap between the best and the second-best score of every root decision it takes, the final move
included: parity of whole trees against an engine whose priors carry float32 error only means something where no decision
was that close."""
import math

import numpy as np

from oracle import chess_py as ch
from oracle import mcts_ref as ref

PURPOSE_GUMBEL = 6            # csrc/gumbel_core.h
DEFAULTS = {"max_considered": 16, "c_visit": 50.0, "c_scale": 1.0}


def considered_visits(m_eff, n):
    """(seq, phase_end) of mctx.get_sequence_of_considered_visits(m_eff, n), built as that function builds it; a phase is a
    maximal run of simulations appended under one number of considered children."""
    if m_eff <= 1:
        return list(range(n)), [n] * n
    log2max = int(math.ceil(math.log2(m_eff)))
    seq, nums = [], []
    visits = [0] * m_eff
    num = m_eff
    while len(seq) < n:
        extra = max(1, int(n / (log2max * num)))
        for _ in range(extra):
            seq.extend(visits[:num])
            nums.extend([num] * num)
            for i in range(num):
                visits[i] += 1
        num = max(2, num // 2)
    seq, nums = seq[:n], nums[:n]
    end = [0] * n
    stop = n
    for s in range(n - 1, -1, -1):
        if s + 1 < n and nums[s + 1] != nums[s]:
            stop = s + 1
        end[s] = stop
    return seq, end


def sigma(q, max_n, c_visit, c_scale):
    return (c_visit + max_n) * c_scale * ((q + 1.0) / 2.0)


def root_stats(prior, q, n, root_v):
    """(max N, v_mix)"""
    vis = [i for i in range(len(n)) if n[i] > 0]
    if not vis:
        return 0, float(root_v)
    sum_n = sum(int(n[i]) for i in vis)
    sum_p = sum(float(prior[i]) for i in vis)
    sum_pq = sum(float(prior[i]) * float(q[i]) for i in vis)
    if not sum_p > 0.0:
        return max(int(n[i]) for i in vis), float(root_v)
    return max(int(n[i]) for i in vis), (float(root_v) + (sum_n / sum_p) * sum_pq) / (1.0 + sum_n)


def scores(prior, q, n, gl, root_v, c_visit, c_scale):
    """(score per child, log prior + sigma per child, v_mix)"""
    max_n, v_mix = root_stats(prior, q, n, root_v)
    bonus = np.array([sigma(float(q[i]) if n[i] > 0 else v_mix, max_n, c_visit, c_scale) for i in range(len(n))], np.float64)
    with np.errstate(divide="ignore"):
        logp = np.log(np.asarray(prior, np.float64))
    return np.asarray(gl, np.float64) + bonus, logp + bonus, v_mix


def improve(prior, q, n, gl, root_v, c_visit=DEFAULTS["c_visit"], c_scale=DEFAULTS["c_scale"]):
    """(pi, v_mix, pick, gap): gap = by how much the pick's score beats the next child with as many visits (inf: none)."""
    sc, logits, v_mix = scores(prior, q, n, gl, root_v, c_visit, c_scale)
    e = np.exp(logits - logits.max())
    pi = e / e.sum()
    top = max(int(x) for x in n)
    cand = [i for i in range(len(n)) if n[i] == top]
    pick = max(cand, key=lambda i: (sc[i], -i))
    rest = [sc[i] for i in cand if i != pick]
    return pi, v_mix, pick, (float(sc[pick] - max(rest)) if rest else math.inf)


def gumbel_draws(stream, k):
    """g_i = -log(-log(u_i)) for the next k draws of the stream, u clamped to [1e-300, 1)"""
    return np.array([-math.log(-math.log(max(stream.next(), 1e-300))) for _ in range(k)], np.float64)


class GumbelMCTS(ref.MCTS):
    """oracle.mcts_ref.MCTS with the Gumbel root: `search` is MCTS.run for a fresh tree in this mode."""

    def __init__(self, cfg, infer, seed=1234, game=0, max_considered=DEFAULTS["max_considered"], c_visit=DEFAULTS["c_visit"],
                 c_scale=DEFAULTS["c_scale"]):
        super().__init__(cfg, infer, seed=seed, game=game)
        self.gumbel = ref.Stream(ref.derive_seed(seed, game, PURPOSE_GUMBEL))
        self.max_considered, self.c_visit, self.c_scale = int(max_considered), float(c_visit), float(c_scale)
        self.min_gap = math.inf
        self.rows = []                      # network rows of every pass, the root's own evaluation first
        self.miss = 0

    # ---- the root level
    def _begin_pass(self, root):
        kids = list(root.children.values())
        self._cnt = [c.n for c in kids]
        self._score = scores([c.prior for c in kids], [c.q for c in kids], self._cnt, self._gl, self._root_v, self.c_visit,
                             self.c_scale)[0]

    def _root_pick(self, want):
        cand = [i for i in range(len(self._cnt)) if self._cnt[i] == want]
        if not cand:
            self.miss += 1
            cand = list(range(len(self._cnt)))
        best = max(cand, key=lambda i: (self._score[i], -i))
        rest = [self._score[i] for i in cand if i != best]
        if rest:
            self.min_gap = min(self.min_gap, float(self._score[best] - max(rest)))
        self._cnt[best] += 1
        return best

    def select(self, board, root, inflight):
        """MCTS.select with the root rule at depth 0: no jitter draw there; below it the parent's scan, line by line."""
        cfg = self.cfg
        node = root
        path = [root]
        while node.expanded:
            if not node.children:
                break
            if node is root:
                best = list(root.children.values())[self._root_pick(self._seq[self._sim])]
            else:
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
            board.push(best.move)
            node = best
            path.append(node)
            if inflight is not None:
                inflight[best] = inflight.get(best, 0) + 1
        self._sim += 1
        return node, path, board

    def run_batched(self, board, root, sims):
        """MCTS.run_batched with passes that end at the phase boundaries of the schedule."""
        L = int(self.cfg.inference_batch_size) or 96
        done = 0
        while done < sims:
            batch_n = min(L, sims - done, self._end[done] - done)
            self._begin_pass(root)
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

    def search(self, board, sims):
        """A fresh tree, no Dirichlet noise, `sims` simulations: {"root", "pi", "v_mix", "pick", "gl", "root_v"}."""
        assert not self.cfg.use_tt and not board.is_game_over()
        root = ref.Node()
        logits, v = self._infer_one(board)
        self.rows.append(1)
        self.expand(root, board, logits, is_root=True)
        kids = list(root.children.values())
        k = len(kids)
        self._root_v = v
        self._gl = gumbel_draws(self.gumbel, k) + np.log(np.array([c.prior for c in kids], np.float64))
        self._seq, self._end = considered_visits(min(self.max_considered, k), sims)
        self._sim = 0
        self.run_batched(board, root, sims)
        pi, v_mix, pick, gap = improve([c.prior for c in kids], [c.q for c in kids], [c.n for c in kids], self._gl, v,
                                       self.c_visit, self.c_scale)
        self.min_gap = min(self.min_gap, gap)
        self._last_root = root
        return {"root": root, "pi": pi, "v_mix": v_mix, "pick": pick, "gl": self._gl.copy(), "root_v": v}
