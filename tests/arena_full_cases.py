"""Searches that run out of node arena: the case table shared by tests/test_node_cap.py (the capped oracle alone, on the CPU) and
tests/test_arena_full_gpu.py (the engine against it).

Every case is one search from a fresh root in an arena of CAP nodes -- the engine's minimum -- with entropy noise and Dirichlet
noise on, fed by HashNet(seed=3).  A row's cases share one engine: virtual loss, leaves per pass, simulations and the network's
sharpness belong to the row.  `conditions` is what a case has to show ON THE ORACLE before a comparison with it means anything:
the cap binds in the middle of the search, often, and (without virtual loss) on leaves that are reached again within the pass."""
from dataclasses import dataclass
from typing import List

from oracle import chess_py as ch
from oracle import mcts_ref as ref
from tests import rules_cases as rc
from tests.hash_net import HashNet
from tests.test_search_gpu import FENS, MCTS          # the search settings and roots of the parity tests

CAP = 4096
SEED = 1234
KIWIPETE, ROOK_ENDGAME = FENS[1], FENS[2]

@dataclass(frozen=True)
class Row:
    name: str
    fens: tuple
    names: tuple
    vl_active: bool
    leaves: int
    sims: int
    sharp: float
    uid0: int

    def net(self):
        return HashNet(seed=3, sharp=self.sharp)


ROWS = [
    Row("vl_16", (ch.START_FEN, KIWIPETE, ROOK_ENDGAME, rc.WIDE_218), ("start", "kiwipete", "rook_endgame", "wide_218"),
        True, 16, 400, 6.0, 2000),
    # (game id 2012: of the ids 2010..2019 the one whose streams make the cap bind most often on this root)
    Row("vl_16_wide138", (rc.WIDE_138,), ("wide_138",), True, 16, 700, 6.0, 2012),
    Row("novl_2", (ch.START_FEN, KIWIPETE, rc.WIDE_218), ("start", "kiwipete", "wide_218"), False, 2, 600, 6.0, 2020),
    # peaked priors: no entropy noise below the root, long narrow lines
    Row("vl_16_sharp30", (KIWIPETE,), ("kiwipete",), True, 16, 400, 30.0, 2030),
    Row("novl_2_sharp30", (ch.START_FEN,), ("start",), False, 2, 600, 30.0, 2040),
    # flat priors: at sharp 6.0 hardly a leaf below the root passes the entropy test, so no refused expansion draws noise and
    # the rule "what a refused expansion drew stays drawn" would go untested; at 3.0 most of them do
    Row("vl_16_sharp3", (KIWIPETE, rc.WIDE_218), ("kiwipete", "wide_218"), True, 16, 400, 3.0, 2050),
    Row("novl_2_sharp3", (KIWIPETE, rc.WIDE_218), ("kiwipete", "wide_218"), False, 2, 600, 3.0, 2060),
]


def oracle_cfg(row: Row, node_cap: int = CAP, **switches) -> ref.MCTSConfig:
    return ref.MCTSConfig.from_dict({**dict(MCTS, use_tt=False, virtual_loss_active=row.vl_active, inference_batch_size=row.leaves,
                                            numerics="engine", node_cap=node_cap), **switches})


def run_oracle(row: Row, g: int, node_cap: int = CAP, cls=ref.MCTS):
    """The oracle's search of case g of `row` -> (MCTS object, visit counts, root q)."""
    o = cls(oracle_cfg(row, node_cap), row.net().infer_np, seed=SEED, game=row.uid0 + g)
    vc, _, rq = o.run(ch.Board(row.fens[g]), num_simulations=row.sims, ply=0)
    return o, vc, rq


@dataclass
class CapFigures:
    attempts: int
    refused: int
    first_refusal: int          # 1-based attempt at which the cap first bound, 0 = never
    fitted_after_refusal: int   # expansions that fitted after the first refusal
    same_pass_retries: int      # refused attempts on a node that the same pass had already been refused


def cap_figures(o: ref.MCTS, search: int = 0) -> CapFigures:
    att = [a for a in o.attempts if a[0] == search]               # (a fresh root's own expansion is the first)
    ok = [a[5] for a in att]
    first = ok.index(False) + 1 if False in ok else 0
    seen, retries = set(), 0
    for (_, p, node, _, _, fitted) in att:
        if not fitted:
            retries += (p, id(node)) in seen
            seen.add((p, id(node)))
    return CapFigures(len(att), ok.count(False), first, sum(ok[first:]) if first else 0, retries)


def conditions(row: Row, f: CapFigures) -> List[str]:
    """What a case misses, in words; empty = it serves."""
    bad = []
    if not (f.first_refusal and 0.10 * f.attempts <= f.first_refusal <= 0.85 * f.attempts):
        bad.append(f"first refusal at attempt {f.first_refusal} of {f.attempts}: not between 10 % and 85 %")
    if f.refused < 6:
        bad.append(f"only {f.refused} expansions refused")
    if not row.vl_active and f.same_pass_retries < 20:
        bad.append(f"only {f.same_pass_retries} retries of a refused leaf within a pass")
    return bad


def tree_nodes(root) -> list:
    out, stack = [], [root]
    while stack:
        node = stack.pop()
        out.append(node)
        stack.extend(node.children.values())
    return out


def reuse_move(root, ply):
    """The move a reuse test plays after the search of `ply`: the most visited root child, on odd plies the least visited of the
    EXPANDED ones (a refused child has visits and no subtree to keep); first of equals."""
    kids = list(root.children.items())
    if ply % 2 == 0:
        return max(kids, key=lambda mc: mc[1].n)[0]
    return min((mc for mc in kids if mc[1].expanded), key=lambda mc: mc[1].n)[0]
