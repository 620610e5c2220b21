"""The oracle's node cap (oracle/mcts_ref.py MCTSConfig.node_cap), the restatement of what the engine does when a search runs out
of node arena (csrc/tree_expand.hip write_children, tree_device.h reroot_*): without a cap nothing changes; with one the tree
keeps the arena's invariants; the case table of tests/arena_full_cases.py makes the cap bind where it has to; and a wrong arena
rule gives other visit counts, so the engine's parity with this oracle (tests/test_arena_full_gpu.py) does pin the rule."""
import functools

import pytest

from oracle import chess_py as ch
from oracle import mcts_ref as ref
from tests import arena_full_cases as ac
from tests import test_search_gpu as sg
from tests.fake_net import FakeNet

CASES = [(row, g) for row in ac.ROWS for g in range(len(row.fens))]
CASE_IDS = [f"{row.name}-{row.names[g]}" for row, g in CASES]


@functools.lru_cache(maxsize=None)
def _capped(row_name, g):
    row = next(r for r in ac.ROWS if r.name == row_name)
    return ac.run_oracle(row, g)


def _tree_signature(root):
    """Every node of the tree in depth-first move order: path, statistics, prior, expansion state."""
    out, stack = [], [((), root)]
    while stack:
        path, node = stack.pop()
        out.append((path, node.n, node.w, node.q, node.prior, node.expanded, node.move_idx, len(node.children)))
        for m, c in reversed(list(node.children.items())):
            stack.append((path + (m.uci(),), c))
    return out


@pytest.mark.parametrize("vl_active,dirichlet,sharp", [(True, True, 8.0), (False, False, 8.0), (True, True, 0.5), (True, False, 30.0)])
def test_without_a_cap_or_below_it_the_search_is_what_it_was(vl_active, dirichlet, sharp):
    """The cases of test_search_gpu.test_search_matches_oracle: node_cap 0 and a cap that never binds give the same tree, node for
    node, the same stream positions and the same evaluation count; `next` counts the tree's nodes and the flag stays clear."""
    L, sims = 8, 96
    m = dict(sg.MCTS, inference_batch_size=L)
    for g, fen in enumerate(sg.FENS):
        runs = []
        for cap in (0, 10**9):
            o, b, vc, pi, rq = sg._oracle(fen, 100 + g, sims, L, FakeNet(seed=3, sharp=sharp), m, vl_active, dirichlet, node_cap=cap)
            assert not o.overflow and all(a[5] for a in o.attempts)
            assert o.next == len(ac.tree_nodes(o._last_root)) == 1 + sum(a[3] for a in o.attempts)
            runs.append((_tree_signature(o._last_root), vc, rq, pi.tolist(), o.evals, o.jitter.ctr, o.noise.ctr, o.dirichlet.ctr))
        assert runs[0] == runs[1], fen


@pytest.mark.parametrize("row,g", CASES, ids=CASE_IDS)
def test_capped_search_keeps_the_arena_invariants(row, g):
    o, vc, rq = _capped(row.name, g)
    root = o._last_root
    assert o.overflow
    nxt = 1
    for (_, _, node, nkeep, before, fitted) in o.attempts:
        assert before == nxt and fitted == (before + nkeep <= ac.CAP)         # per expansion, on the block after pruning
        nxt += nkeep if fitted else 0
        assert nxt <= ac.CAP
    assert o.next == nxt == len(ac.tree_nodes(root))                          # the reachable nodes are the arena's, all of them
    assert sum(vc.values()) == row.sims == root.n                            # no simulation lost to a refusal
    fitted_later = {id(a[2]) for a in o.attempts if a[5]}
    refused = [a[2] for a in o.attempts if not a[5] and id(a[2]) not in fitted_later]
    assert refused
    for node in refused:
        assert node.n > 0 and not node.expanded and not node.children


def test_case_table_makes_the_cap_bind_where_it_has_to(capsys):
    later = 0
    with capsys.disabled():
        print()
        for row, g in CASES:
            o, _, _ = _capped(row.name, g)
            f = ac.cap_figures(o)
            print(f"node cap {ac.CAP} [{row.name}/{row.names[g]}]: first refusal at attempt {f.first_refusal} of {f.attempts}, "
                  f"{f.refused} refused, {f.fitted_after_refusal} fitted after it, {f.same_pass_retries} same-pass retries, "
                  f"next {o.next}")
            assert not ac.conditions(row, f), (row.name, row.names[g], ac.conditions(row, f))
            later += f.fitted_after_refusal > 0
    assert later >= 3, later


class _RefusesBeforeTheNoise(ref.MCTS):
    """Wrong rule: the arena test comes before the priors, so a refused expansion draws nothing from the noise stream."""

    def expand(self, node, board, logits, is_root=False):
        nkeep = len(ch.legal_moves_with_indices(board)[0])                    # (no pruning in the case table)
        if not node.expanded and self.cfg.node_cap and self.next + nkeep > self.cfg.node_cap:
            self.claim_nodes(node, nkeep)
            return
        super().expand(node, board, logits, is_root)


class _RefusesForGood(ref.MCTS):
    """Wrong rule: after the first refusal nothing fits any more."""

    def claim_nodes(self, node, nkeep):
        return super().claim_nodes(node, ac.CAP + 1 if self.overflow else nkeep)


@pytest.mark.parametrize("wrong", [_RefusesBeforeTheNoise, _RefusesForGood])
def test_a_wrong_arena_rule_changes_the_visit_counts(wrong):
    differ = []
    for row, g in CASES:
        o, vc, _ = _capped(row.name, g)
        ow, vcw, _ = ac.run_oracle(row, g, cls=wrong)
        assert ow.overflow
        if list(vcw.values()) != list(vc.values()):
            differ.append(f"{row.name}/{row.names[g]}")
    print(f"{wrong.__name__}: other root visit counts in {differ}")
    assert differ


def test_cap_binds_again_after_every_reroot():
    """note_move_played + run: `next` starts at the size of the kept subtree, unvisited children included, and the flag is the new
    search's own."""
    row = ac.ROWS[0]
    o = ref.MCTS(ac.oracle_cfg(row), row.net().infer_np, seed=ac.SEED, game=row.uid0 + 1)
    b = ch.Board(row.fens[1])
    for ply in range(3):
        vc, _, _ = o.run(b, num_simulations=row.sims, ply=ply)
        root = o._last_root
        assert o.overflow and o.next <= ac.CAP and o.next == len(ac.tree_nodes(root))
        if ply:
            assert o.next_at_start == kept and 1 < kept < ac.CAP
            assert [a[5] for a in o.attempts if a[0] == ply][0]               # expansion resumed: the flag did not carry over
        mv = ac.reuse_move(root, ply)
        kept = len(ac.tree_nodes(root.children[mv]))
        o.note_move_played(mv)
        b.push(mv)
