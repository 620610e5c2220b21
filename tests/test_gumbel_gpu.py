"""The Gumbel root search on the GPU (include/m0_gumbel.h: csrc/tree_gumbel.h in select_kernel and expand_kernel) against
tests/gumbel_ref.py, through the split-step search with the evaluators of tests/test_search_gpu.py, and end to end in self-play.

Visit counts, move order, the move taken and the rows of every pass must be identical; pi, v_mix and gl within 1e-9, the
project's fp64 tolerance.  The engine's priors carry float32 rounding (1e-6 in the existing tests), so a root decision that the
reference takes by less than 1e-4 could fall either way: the seeds here were chosen, with the reference alone, so that no case
has one, and every case asserts it."""
import functools

import numpy as np
import pytest

from oracle import chess_py as ch
from oracle import mcts_ref as ref
from tests import gumbel_ref as gr
from tests import rules_cases as rc
from tests.fake_net import FakeNet
from tests.hash_net import HashNet
from tests.test_search_gpu import FENS, MCTS

pytestmark = pytest.mark.gpu

SEED = 1234
MIN_GAP = 1e-4
SWEEP = [(16, 16), (5, 16), (24, 4), (64, 16), (33, 3)]          # (simulations, max_considered)
ONE_MOVE = "rnbqkb1r/p1pppQ2/1p3n1p/5pp1/1P6/2P2P2/P2PP1PP/RNBK1BNR b kq - 1 8"      # Kxf7 is all there is
THREE_MOVES = "B2k1R2/8/1N4pn/p1b1p3/4b1P1/prPPP3/5P1N/2BQ1K2 b - - 2 31"


def _engine(G, L, sims, vl_active, gumbel, compat=None):
    from matrix0_amd import engine as eng
    m = dict(MCTS, inference_batch_size=L)
    cfg = eng.selfplay_cfg_from_dict({"seed": SEED, "mcts": m, "selfplay": {"num_simulations": sims}}, concurrent_games=G,
                                     virtual_loss_active=vl_active, compat=compat)
    e = eng.SelfplayEngine(None, cfg)
    if gumbel is not None:
        e.set_gumbel(**gumbel)
    return e, m


def _run(e, net, G):
    """All searches to their end: (results, Gumbel results, rows of every pass over all slots)"""
    rows = []
    for _ in range(1000):
        planes = e.search_select()
        rows.append(int(planes.shape[0]))
        lg, v = net.infer_np(planes) if planes.shape[0] else (np.zeros((0, 4672), np.float32), np.zeros((0,), np.float32))
        e.search_expand(lg, v)
        if all(e.search_result(g)["finished"] for g in range(G)):
            break
    return [e.search_result(g) for g in range(G)], [e.search_gumbel_result(g) for g in range(G)], rows


def _reference(fen, uid, sims, L, net, m, vl_active, gumbel):
    cfg = ref.MCTSConfig.from_dict(dict(m, use_tt=False, virtual_loss_active=vl_active, inference_batch_size=L, numerics="engine"))
    o = gr.GumbelMCTS(cfg, net.infer_np, seed=SEED, game=uid, **gumbel)
    o._uid = uid
    return o, o.search(ch.Board(fen), sims)


def _rows_of_all(oracles):
    n = max(len(o.rows) for o in oracles)
    return [sum(o.rows[p] for o in oracles if p < len(o.rows)) for p in range(n)]


def _check(res, gres, o, want, net, fen, gumbel):
    kids = list(want["root"].children.values())
    assert o.miss == 0 and o.min_gap >= MIN_GAP, f"a root decision by {o.min_gap}: choose another seed for this case"
    assert gres["miss"] == 0
    assert res["moves"] == [c.move.uci() for c in kids]
    assert res["n"].tolist() == [c.n for c in kids], (res["n"].tolist(), [c.n for c in kids])
    assert gres["pick"] == want["pick"]
    np.testing.assert_allclose(res["prior"], [c.prior for c in kids], rtol=0, atol=1e-6)
    np.testing.assert_allclose(res["q"], [c.q for c in kids], rtol=0, atol=1e-6)
    # the functions, on the engine's own statistics: the root's value is the evaluator's, as the engine clips it
    _, v = net.infer_np(ch.encode_board(ch.Board(fen))[None])
    root_v = float(np.clip(np.float64(v[0]), -1.0, 1.0))
    assert root_v == want["root_v"]
    pi, v_mix, pick, _ = gr.improve(res["prior"], res["q"], res["n"], gres["gl"], root_v, gumbel["c_visit"], gumbel["c_scale"])
    np.testing.assert_allclose(gres["pi"], pi, rtol=0, atol=1e-9)
    assert abs(gres["v_mix"] - v_mix) <= 1e-9 and gres["pick"] == pick
    assert abs(gres["pi"].sum() - 1.0) <= 1e-9 and np.all(gres["pi"] > 0)
    # gl = g + log(prior) with the game's stream: the first k draws of a slot's first search
    g = gr.gumbel_draws(ref.Stream(ref.derive_seed(SEED, o._uid, gr.PURPOSE_GUMBEL)), len(kids))
    np.testing.assert_allclose(gres["gl"], g + np.log(res["prior"]), rtol=0, atol=1e-9)


def _uid(case, g):
    return 1000 + 10 * case + g


def _case_index(sims, m, L, vl):
    return (SWEEP.index((sims, m)) * 2 + [8, 96].index(L)) * 2 + int(vl)


@functools.lru_cache(maxsize=None)
def sweep_reference(sims, m, L, vl):
    """The six reference searches of one case, computed once."""
    gumbel = dict(gr.DEFAULTS, max_considered=m)
    out = []
    for g, fen in enumerate(FENS):
        out.append(_reference(fen, _uid(_case_index(sims, m, L, vl), g), sims, L, FakeNet(seed=3, sharp=8.0),
                              dict(MCTS, inference_batch_size=L), vl, gumbel))
    return out


@pytest.mark.parametrize("vl", [True, False])
@pytest.mark.parametrize("L", [8, 96])
@pytest.mark.parametrize("sims,m", SWEEP)
def test_tree_and_functions_match_the_reference(sims, m, L, vl):
    """The six positions of test_search_gpu.py; two of them put mate and stalemate leaves directly under the root, where the
    in-flight count and the immediate backup would count a visit twice."""
    G = len(FENS)
    gumbel = dict(gr.DEFAULTS, max_considered=m)
    want = sweep_reference(sims, m, L, vl)
    e, _ = _engine(G, L, sims, vl, gumbel)
    net = FakeNet(seed=3, sharp=8.0)
    for g, fen in enumerate(FENS):
        e.search_begin(g, fen, sims, True, want[g][0]._uid)        # Dirichlet asked for: the mode ignores it
    results, gresults, rows = _run(e, net, G)
    e.close()
    assert rows == _rows_of_all([o for o, _ in want]), (rows, [o.rows for o, _ in want])
    for g, fen in enumerate(FENS):
        _check(results[g], gresults[g], want[g][0], want[g][1], net, fen, gumbel)
        assert int(results[g]["n"].sum()) == sims


NARROW_WIDE = [(ONE_MOVE, 1, 16, 12, 8), (THREE_MOVES, 3, 16, 20, 8), (rc.WIDE_218, 218, 128, 160, 96), (rc.WIDE_138, 138, 128, 140, 16)]


def test_narrow_and_wide_roots():
    """Fewer root children than max_considered (1 and 3), and more than one wave of them at max_considered = 128."""
    for j, (fen, k, m, sims, L) in enumerate(NARROW_WIDE):
        assert len(ch.legal_moves_with_indices(ch.Board(fen))[0]) == k, fen
        gumbel = dict(gr.DEFAULTS, max_considered=m)
        uid = 2000 + j
        e, mm = _engine(1, L, sims, True, gumbel)
        net = HashNet(seed=41, sharp=6.0)
        o, want = _reference(fen, uid, sims, L, HashNet(seed=41, sharp=6.0), mm, True, gumbel)
        e.search_begin(0, fen, sims, False, uid)
        results, gresults, rows = _run(e, net, 1)
        e.close()
        assert rows == o.rows, (fen, rows, o.rows)
        assert len(results[0]["n"]) == k
        _check(results[0], gresults[0], o, want, net, fen, gumbel)
        if k > 64:
            assert np.count_nonzero(results[0]["n"][64:]) > 0, "no visit went past the first wave of children"


def test_a_second_search_of_a_slot_starts_fresh_and_draws_on():
    """search_advance in this mode: a fresh tree whatever the slot held, and the next k draws of the game's stream."""
    sims, L, uid = 16, 8, 3000
    gumbel = dict(gr.DEFAULTS)
    e, m = _engine(1, L, sims, True, gumbel)
    net = FakeNet(seed=3, sharp=8.0)
    cfg = ref.MCTSConfig.from_dict(dict(m, use_tt=False, virtual_loss_active=True, inference_batch_size=L, numerics="engine"))
    o = gr.GumbelMCTS(cfg, FakeNet(seed=3, sharp=8.0).infer_np, seed=SEED, game=uid, **gumbel)
    b = ch.Board(FENS[1])
    e.search_begin(0, FENS[1], sims, False, uid)
    for ply in range(2):
        results, gresults, _ = _run(e, net, 1)
        want = o.search(b, sims)
        kids = list(want["root"].children.values())
        assert o.min_gap >= MIN_GAP
        assert results[0]["n"].tolist() == [c.n for c in kids] and int(results[0]["root_n"]) == sims
        assert gresults[0]["pick"] == want["pick"] and gresults[0]["miss"] == 0
        np.testing.assert_allclose(gresults[0]["gl"], want["gl"], rtol=0, atol=1e-9)
        np.testing.assert_allclose(gresults[0]["pi"], want["pi"], rtol=0, atol=1e-6)      # the reference's own priors: float32 error
        b.push(kids[want["pick"]].move)
        if ply == 0:
            e.search_advance(0, want["pick"], sims, False)
    e.close()


SP_CFG = {"seed": 77,
          "mcts": dict(MCTS, inference_batch_size=8),
          "selfplay": {"num_simulations": 16, "max_game_len": 5, "min_resign_plies": 500, "opening_random_plies": 0,
                       "temperature_start": 1.0, "temperature_end": 1.0, "temperature_moves": 40}}


def _selfplay(cfg_dict, gumbel, games=3):
    from matrix0_amd import engine as eng
    e = eng.SelfplayEngine(None, eng.selfplay_cfg_from_dict(cfg_dict, concurrent_games=games, total_games=games))
    if gumbel is not None:
        e.set_gumbel(gumbel)
    net = HashNet(seed=51, sharp=6.0)
    out = {}
    for _ in range(2000):
        if not e.running():
            break
        planes = e.ext_select()
        lg, v = net.infer_np(planes) if planes.shape[0] else (np.zeros((0, 4672), np.float32), np.zeros((0,), np.float32))
        e.ext_expand(lg, v)
        while (r := e.poll()) is not None:
            out[r["game_index"]] = r
    e.close()
    assert sorted(out) == list(range(games))
    return out


def test_selfplay_records_the_improved_policy_and_plays_the_pick():
    from matrix0_amd import engine as eng
    cfg_dict = dict(SP_CFG, mcts=dict(SP_CFG["mcts"], gumbel={"enabled": True}))
    gumbel = eng.gumbel_cfg_from_dict(cfg_dict)
    runs = [_selfplay(cfg_dict, gumbel) for _ in range(2)]
    for g in runs[0]:
        assert runs[0][g]["played"] == runs[1][g]["played"], g
        for key in ("pi", "z", "search_values", "s", "legal_mask"):
            assert np.array_equal(runs[0][g][key], runs[1][g][key]), (g, key)
    mcfg = ref.MCTSConfig.from_dict(dict(SP_CFG["mcts"], use_tt=False, virtual_loss_active=True, numerics="engine"))
    for g, rec in runs[0].items():
        T = rec["moves"]
        assert T == 5 and len(rec["played"]) == 5
        np.testing.assert_allclose(rec["pi"].sum(axis=1), 1.0, rtol=0, atol=1e-5)
        assert np.all(rec["pi"][rec["legal_mask"] == 0] == 0)
        assert np.all(rec["pi"][rec["legal_mask"] == 1] > 0), "visit counts of 16 simulations cannot cover every legal move"
        # every ply again with the reference, whose streams run on through the game as the slot's do
        o = gr.GumbelMCTS(mcfg, HashNet(seed=51, sharp=6.0).infer_np, seed=77, game=g)
        b = ch.Board()
        for t in range(T):
            want = o.search(b, 16)
            kids = list(want["root"].children.values())
            assert o.min_gap >= MIN_GAP, f"game {g} ply {t}: a root decision by {o.min_gap}"
            assert rec["played"][t] == kids[want["pick"]].move.uci(), (g, t)
            pi = np.zeros(4672, np.float64)
            pi[[c.move_idx for c in kids]] = want["pi"]
            np.testing.assert_allclose(rec["pi"][t], pi, rtol=0, atol=1e-6)      # float32 rows; the priors are the same float32 values
            assert abs(rec["search_values"][t] - want["root"].q) <= 1e-6
            b.push(kids[want["pick"]].move)


def test_an_engine_without_the_call_plays_as_one_without_the_block():
    with_block = dict(SP_CFG, mcts=dict(SP_CFG["mcts"], gumbel={"enabled": True, "max_considered": 4}))
    a, b = _selfplay(with_block, None), _selfplay(SP_CFG, None)
    for g in a:
        assert a[g]["played"] == b[g]["played"], g
        for key in ("pi", "z", "search_values", "s", "legal_mask"):
            assert np.array_equal(a[g][key], b[g][key]), (g, key)
    # and those are PUCT games: visit-count targets, which leave legal moves without mass at this budget
    assert all(np.any(a[g]["pi"][a[g]["legal_mask"] == 1] == 0) for g in a)


def test_the_setter_says_when_and_where_it_cannot_be_used():
    from matrix0_amd import engine as eng
    cfg = eng.selfplay_cfg_from_dict({"seed": 1, "mcts": dict(MCTS, inference_batch_size=8), "selfplay": {"num_simulations": 8}},
                                     concurrent_games=1)
    e = eng.SelfplayEngine(None, cfg)
    for bad in [dict(max_considered=0), dict(max_considered=257), dict(c_visit=-1.0), dict(c_scale=float("nan")),
                dict(c_visit=float("inf"))]:
        with pytest.raises(ValueError):
            e.set_gumbel(**bad)
    with pytest.raises(RuntimeError, match="not set"):
        e.search_gumbel_result(0)
    e.set_gumbel(max_considered=256)
    e.set_gumbel()                                              # again, before the first search: the last one holds
    e.search_begin(0, ch.START_FEN, 8, False, 0)
    assert e.search_gumbel_result(0)["pick"] == -1              # not finished
    with pytest.raises(RuntimeError, match="before the first"):
        e.set_gumbel()
    e.close()
    e = eng.SelfplayEngine(None, eng.selfplay_cfg_from_dict({"selfplay": {"num_simulations": 8}}, concurrent_games=1,
                                                             compat={"tt_merge": True}))
    with pytest.raises(ValueError, match="tt_merge"):
        e.set_gumbel()
    e.close()
    for other in (eng.ArenaExtEngine(cfg), eng.AnalysisExtEngine(cfg)):
        with pytest.raises(RuntimeError, match="self-play engines only"):
            other.set_gumbel()
        other.close()
