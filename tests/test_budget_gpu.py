"""The self-play budget mix on the GPU (include/m0_budget.h: the forced instantiation of select_kernel, csrc/tree_forced.h, and the
game loop's full and fast searches) against tests/budget_ref.py, through the split-step search and the external-evaluator
self-play loop with the host evaluators of tests/test_search_gpu.py: no network kernel runs.

Visit counts, move order, rows of every pass, evaluation counts and forced descents must be identical; pruned counts identical
and their pi within 1e-15.  A deficit test that the reference decides by less than 1e-9 (relative) or a pruning test by less
than 1e-7 could fall either way on statistics that differ in their last bits: the seeds and positions here were chosen, with
the reference alone, so that no case has one, and every case asserts it before it compares.  No case is left out."""
import functools

import numpy as np
import pytest

from oracle import chess_py as ch
from oracle import mcts_ref as ref
from tests import budget_ref as br
from tests.fake_net import FakeNet
from tests.hash_net import HashNet
from tests.test_search_gpu import FENS, MCTS

pytestmark = pytest.mark.gpu

SEED = 1234
THREE_MOVES = "B2k1R2/8/1N4pn/p1b1p3/4b1P1/prPPP3/5P1N/2BQ1K2 b - - 2 31"
# a wide middlegame root (48 moves), a root with 3 moves, mate and stalemate leaves directly under the root, a quiet middlegame
SEARCH_FENS = [FENS[1], THREE_MOVES, FENS[5], FENS[3]]
NOISE = True                                                    # Dirichlet noise on: P_i is the prior after noise


def _engine(G, L, sims, vl_active, budget, compat=None, seed=SEED):
    from matrix0_amd import engine as eng
    m = dict(MCTS, inference_batch_size=L)
    cfg = eng.selfplay_cfg_from_dict({"seed": seed, "mcts": m, "selfplay": {"num_simulations": sims}}, concurrent_games=G,
                                     virtual_loss_active=vl_active, compat=compat)
    e = eng.SelfplayEngine(None, cfg)
    if budget is not None:
        e.set_budget(**budget)
    return e, m


def _run(e, net, G):
    """All searches to their end: (results, budget results, rows of every pass over all slots)"""
    rows = []
    for _ in range(1000):
        planes = e.search_select()
        rows.append(int(planes.shape[0]))
        lg, v = net.infer_np(planes) if planes.shape[0] else (np.zeros((0, 4672), np.float32), np.zeros((0,), np.float32))
        e.search_expand(lg, v)
        if all(e.search_result(g)["finished"] for g in range(G)):
            break
    return [e.search_result(g) for g in range(G)], [e.search_budget_result(g) for g in range(G)], rows


def _oracle(uid, L, net, vl_active):
    cfg = ref.MCTSConfig.from_dict(dict(MCTS, use_tt=False, virtual_loss_active=vl_active, inference_batch_size=L,
                                        dirichlet_plies=30, numerics="engine"))
    return br.BudgetMCTS(cfg, net.infer_np, seed=SEED, game=uid)


def _uid(sims, L, vl, forced_k, g):
    case = (([64, 200].index(sims) * 2 + [8, 32].index(L)) * 2 + int(vl)) * 2 + [0.5, 2.0].index(forced_k)
    return 5000 + 10 * case + g


@functools.lru_cache(maxsize=None)
def sweep_reference(sims, L, vl, forced_k):
    """The four reference searches of one case, computed once: [(oracle, root children)]"""
    out = []
    for g, fen in enumerate(SEARCH_FENS):
        o = _oracle(_uid(sims, L, vl, forced_k, g), L, FakeNet(seed=3, sharp=8.0), vl)
        out.append((o, o.search(ch.Board(fen), sims, ply=0, forced_k=forced_k)))
    return out


def _rows_of_all(oracles):
    n = max(len(o.rows) for o in oracles)
    return [sum(o.rows[p] for o in oracles if p < len(o.rows)) for p in range(n)]


def _check_tree(res, o, kids):
    assert o.min_deficit_margin >= br.MIN_DEFICIT_MARGIN, f"a deficit test by {o.min_deficit_margin}: choose another seed"
    assert res["moves"] == [c.move.uci() for c in kids]
    assert res["n"].tolist() == [c.n for c in kids], (res["n"].tolist(), [c.n for c in kids])
    np.testing.assert_allclose(res["prior"], [c.prior for c in kids], rtol=0, atol=1e-6)
    np.testing.assert_allclose(res["q"], [c.q for c in kids], rtol=0, atol=1e-6)
    assert res["root_n"] == o._last_root.n


def _check_pruned(res, bres, cpuct, forced_k):
    """search_budget_result against the reference's pruning of the engine's own statistics"""
    want_n, want_pi, _, margin = br.prune(res["prior"], res["q"], res["n"], res["root_n"], cpuct, forced_k)
    assert margin >= br.MIN_PRUNE_MARGIN, f"a pruning test by {margin}: choose another seed"
    assert bres["pruned_n"].tolist() == want_n.tolist()
    np.testing.assert_allclose(bres["pi"], want_pi, rtol=0, atol=1e-15)
    return int(res["n"].sum() - want_n.sum())


@pytest.mark.parametrize("forced_k", [0.5, 2.0])
@pytest.mark.parametrize("vl", [True, False])
@pytest.mark.parametrize("L", [8, 32])
@pytest.mark.parametrize("sims", [64, 200])
def test_forced_search_and_pruned_targets_match_the_reference(sims, L, vl, forced_k):
    G = len(SEARCH_FENS)
    want = sweep_reference(sims, L, vl, forced_k)
    e, _ = _engine(G, L, sims, vl, dict(full_prob=1.0, fast_simulations=1, forced_k=forced_k, prune_targets=True))
    net = FakeNet(seed=3, sharp=8.0)
    for g, fen in enumerate(SEARCH_FENS):
        e.search_begin(g, fen, sims, NOISE, _uid(sims, L, vl, forced_k, g))
    results, bresults, rows = _run(e, net, G)
    evals = int(e.stats()["evals"])
    forced = e.budget_stats()["forced_descents"]
    e.close()
    assert rows == _rows_of_all([o for o, _ in want]), (rows, [o.rows for o, _ in want])
    assert evals == sum(o.evals for o, _ in want)
    pruned = 0
    for g in range(G):
        o, kids = want[g]
        _check_tree(results[g], o, kids)
        assert int(results[g]["n"].sum()) == sims
        assert bresults[g]["forced_descents"] == o.forced_descents, (g, bresults[g]["forced_descents"], o.forced_descents)
        pruned += _check_pruned(results[g], bresults[g], o.cpuct_at(0), forced_k)
    assert forced == sum(o.forced_descents for o, _ in want)
    # the rule decided descents in this case (a sweep in which it never does would compare two PUCT searches), and at
    # forced_k = 2 the pruning took visits out again
    assert forced > 0
    if forced_k == 2.0:
        assert pruned > 0


def test_a_second_search_of_a_slot_keeps_the_subtree_and_the_rule():
    """search_advance: the played child's subtree is kept, its visits count towards N, noise is applied again, and the slot's
    count of forced descents runs on."""
    sims, L, uid, forced_k = 64, 8, 5900, 2.0
    e, _ = _engine(1, L, sims, True, dict(full_prob=1.0, fast_simulations=1, forced_k=forced_k, prune_targets=True))
    net = FakeNet(seed=3, sharp=8.0)
    o = _oracle(uid, L, FakeNet(seed=3, sharp=8.0), True)
    b = ch.Board(FENS[1])
    e.search_begin(0, FENS[1], sims, NOISE, uid)
    for ply in range(2):
        results, bresults, _ = _run(e, net, 1)
        kids = o.search(b, sims, ply=ply, forced_k=forced_k)
        _check_tree(results[0], o, kids)
        assert bresults[0]["forced_descents"] == o.forced_descents
        _check_pruned(results[0], bresults[0], o.cpuct_at(0), forced_k)
        if ply == 0:
            pick = int(np.argmax(results[0]["n"]))
            assert kids[pick].n > 1, "the kept subtree has to carry visits"
            b.push(kids[pick].move)
            o.note_move_played(kids[pick].move)
            e.search_advance(0, pick, sims, NOISE)
            first = o.forced_descents
    assert o.forced_descents > first > 0
    e.close()


GAME_CFG = {"seed": 77,
            "mcts": dict(MCTS, inference_batch_size=8),
            "selfplay": {"num_simulations": 48, "max_game_len": 24, "min_resign_plies": 500, "opening_random_plies": 0,
                         "temperature_start": 1.0, "temperature_end": 1.0, "temperature_moves": 40}}
GAME_BUDGET = {"full_prob": 0.5, "fast_simulations": 12, "forced_k": 2.0, "prune_targets": True}


def _selfplay(cfg_dict, budget, games=3, slots=3):
    from matrix0_amd import engine as eng
    e = eng.SelfplayEngine(None, eng.selfplay_cfg_from_dict(cfg_dict, concurrent_games=slots, total_games=games))
    if budget is not None:
        e.set_budget(**budget)
    net = HashNet(seed=51, sharp=6.0)
    out = {}
    for _ in range(20000):
        if not e.running():
            break
        planes = e.ext_select()
        lg, v = net.infer_np(planes) if planes.shape[0] else (np.zeros((0, 4672), np.float32), np.zeros((0,), np.float32))
        e.ext_expand(lg, v)
        while (r := e.poll()) is not None:
            out[r["game_index"]] = r
    st = e.stats()
    bst = e.budget_stats() if budget is not None else None
    e.close()
    assert sorted(out) == list(range(games))
    return out, st, bst


@functools.lru_cache(maxsize=None)
def game_reference(g):
    return br.play_game(GAME_CFG, HashNet(seed=51, sharp=6.0).infer_np, GAME_CFG["seed"], g, GAME_BUDGET)


def _same_games(a, b, keys=("pi", "z", "search_values", "s", "legal_mask")):
    assert sorted(a) == sorted(b)
    for g in a:
        assert a[g]["played"] == b[g]["played"], g
        for key in keys:
            assert np.array_equal(a[g][key], b[g][key]), (g, key)


def test_whole_games_match_the_reference_loop():
    from matrix0_amd import engine as eng
    (run1, st1, bst1), (run2, _, bst2) = _selfplay(GAME_CFG, GAME_BUDGET), _selfplay(GAME_CFG, GAME_BUDGET)
    two_slots, _, bst3 = _selfplay(GAME_CFG, GAME_BUDGET, slots=2)
    keys = ("pi", "z", "search_values", "s", "legal_mask", "full", "sims")
    _same_games(run1, run2, keys)                                    # two runs are bit-identical
    _same_games(run1, two_slots, keys)                               # ... and so are 3 and 2 resident slots
    assert bst1 == bst2 == bst3
    p = GAME_BUDGET["full_prob"]
    n_full = n_fast = forced = 0
    for g, rec in run1.items():
        want = game_reference(g)
        assert want["deficit_margin"] >= br.MIN_DEFICIT_MARGIN and want["prune_margin"] >= br.MIN_PRUNE_MARGIN, \
            f"game {g}: a decision by {want['deficit_margin']} / {want['prune_margin']}: choose another seed"
        T = rec["moves"]
        assert rec["played"] == want["played"], g
        assert T == len(want["full"]) and rec["full"].tolist() == want["full"] and rec["sims"].tolist() == want["sims"]
        assert rec["full"].tolist() == [eng.budget_is_full(GAME_CFG["seed"], g, i, p) for i in range(T)]
        assert set(rec["sims"][rec["full"]].tolist()) <= {48} and set(rec["sims"][~rec["full"]].tolist()) <= {12}
        np.testing.assert_allclose(rec["pi"], want["pi"], rtol=0, atol=1e-6)
        np.testing.assert_allclose(rec["z"], want["z"], rtol=0, atol=1e-6)
        np.testing.assert_allclose(rec["pi"].sum(axis=1), 1.0, rtol=0, atol=1e-5)
        n_full += int(rec["full"].sum()); n_fast += int((~rec["full"]).sum()); forced += want["forced_descents"]
    assert n_full > 0 and n_fast > 0, "the games have to mix both kinds of search"
    assert (bst1["full_searches"], bst1["fast_searches"]) == (n_full, n_fast)
    assert bst1["forced_descents"] == forced > 0 and bst1["pruned_visits"] > 0
    assert int(st1["sims"]) == sum(int(r["sims"].sum()) for r in run1.values())


SHORT_CFG = dict(GAME_CFG, selfplay=dict(GAME_CFG["selfplay"], num_simulations=16, max_game_len=6))


def test_off_is_off():
    # an engine without the call does not see the block
    with_block = dict(SHORT_CFG, mcts=dict(SHORT_CFG["mcts"], budget={"enabled": True, "full_prob": 0.5}))
    (a, st_a, _), (b, st_b, _) = _selfplay(with_block, None), _selfplay(SHORT_CFG, None)
    _same_games(a, b)
    assert "full" not in a[0] and "sims" not in a[0]
    # the mode with every move a full search, no forcing and no pruning plays the same games, through the forced instantiation
    c, st_c, bst = _selfplay(SHORT_CFG, {"full_prob": 1.0, "fast_simulations": 1, "forced_k": 0.0, "prune_targets": False})
    _same_games(b, c)
    for key in ("sims", "evals", "plies", "steps", "games_finished"):
        assert st_a[key] == st_b[key] == st_c[key], key
    assert all(r["full"].all() and set(r["sims"].tolist()) == {16} for r in c.values())
    plies = sum(r["moves"] for r in c.values())
    assert bst == {"full_searches": bst["full_searches"], "fast_searches": 0, "forced_descents": 0, "pruned_visits": 0}
    assert bst["full_searches"] == plies


def test_the_setter_says_when_and_where_it_cannot_be_used():
    from matrix0_amd import engine as eng
    cfg = eng.selfplay_cfg_from_dict({"seed": 1, "mcts": dict(MCTS, inference_batch_size=8), "selfplay": {"num_simulations": 8}},
                                     concurrent_games=1)
    e = eng.SelfplayEngine(None, cfg)
    for bad in [dict(full_prob=0.0), dict(full_prob=1.5), dict(full_prob=float("nan")), dict(fast_simulations=0),
                dict(forced_k=-1.0), dict(forced_k=float("nan")), dict(forced_k=float("inf"))]:
        with pytest.raises(ValueError):
            e.set_budget(**bad)
    with pytest.raises(ValueError):
        e.set_budget(eng.BudgetCfg(0.5, 10, 2.0, 2))
    with pytest.raises(RuntimeError, match="not set"):
        e.search_budget_result(0)
    with pytest.raises(RuntimeError, match="not set"):
        e.budget_stats()
    e.set_budget(full_prob=1.0)
    e.set_budget()                                              # again, before the first search: the last one holds
    for other in (e.set_gumbel, e.set_proof):                   # the other modes refuse an engine in this one
        with pytest.raises(ValueError, match="budget"):
            other()
    e.search_begin(0, ch.START_FEN, 8, False, 0)
    early = e.search_budget_result(0)                           # not finished: -1 and zeros
    assert early["forced_descents"] == -1 and not early["pruned_n"].any() and not early["pi"].any()
    with pytest.raises(RuntimeError, match="before the first"):
        e.set_budget()
    e.close()
    # ... and this one refuses an engine in one of theirs, and the position table
    for first, word in (("set_gumbel", "Gumbel"), ("set_proof", "proof")):
        e = eng.SelfplayEngine(None, cfg)
        getattr(e, first)()
        with pytest.raises(ValueError, match=word):
            e.set_budget()
        e.close()
    e = eng.SelfplayEngine(None, eng.selfplay_cfg_from_dict({"selfplay": {"num_simulations": 8}}, concurrent_games=1,
                                                             compat={"tt_merge": True}))
    with pytest.raises(ValueError, match="tt_merge"):
        e.set_budget()
    e.close()
    for other in (eng.ArenaExtEngine(cfg), eng.AnalysisExtEngine(cfg)):
        with pytest.raises(RuntimeError, match="self-play engines only"):
            other.set_budget()
        other.close()
    # once games have started
    e = eng.SelfplayEngine(None, eng.selfplay_cfg_from_dict(SHORT_CFG, concurrent_games=1, total_games=1))
    planes = e.ext_select()
    lg, v = HashNet(seed=51, sharp=6.0).infer_np(planes)
    e.ext_expand(lg, v)
    with pytest.raises(RuntimeError, match="before the first"):
        e.set_budget()
    e.close()
