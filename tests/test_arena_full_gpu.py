"""Searches that run out of node arena, on the GPU: csrc/tree_expand.hip write_children refuses a child block that does not fit,
the leaf stays unexpanded, the value is backed up, the simulation counts and GameDev::overflow is set until the slot's next root
(tree_device.h reroot_*).  Every engine here has arena_nodes = 4096, the smallest the library allows; the expectation is the
oracle with the same cap (oracle/mcts_ref.py MCTSConfig.node_cap, pinned on its own by tests/test_node_cap.py) on the case table
of tests/arena_full_cases.py.  Tolerances are those of tests/test_search_gpu.py: integers identical, priors and q within 1e-6;
where two runs of the engine are compared (fused against split step, evaluation cache on against off) everything is bit for bit."""
import functools

import numpy as np
import pytest

from oracle import chess_py as ch
from oracle import mcts_ref as ref
from oracle import net_ref
from tests import arena_full_cases as ac
from tests import test_eval_cache_gpu as ecg
from tests import test_search_gpu as sg
from tests import test_timed_path_gpu as tp
from tests.test_analysis_gpu import _oracle_lines

pytestmark = pytest.mark.gpu

ROW_IDS = [row.name for row in ac.ROWS]
MULTIPV, PV_LEN = 8, 16


@functools.lru_cache(maxsize=None)
def _want(row_name, g, cap=ac.CAP):
    """The oracle's search of a case (computed once, never modified)."""
    row = next(r for r in ac.ROWS if r.name == row_name)
    return ac.run_oracle(row, g, node_cap=cap)


def _search_row(row, arena_nodes, **cfg_kw):
    G = len(row.fens)
    e, _ = sg._engine(G, row.leaves, row.sims, vl_active=row.vl_active, arena_nodes=arena_nodes, **cfg_kw)
    net = row.net()
    for g, fen in enumerate(row.fens):
        e.search_begin(g, fen, row.sims, True, row.uid0 + g)
    results = sg._run_engine_search(e, net, G)
    st = e.stats()
    e.close()
    return results, net, st


@pytest.mark.parametrize("row", ac.ROWS, ids=ROW_IDS)
def test_searches_in_a_full_arena_match_the_capped_oracle(row):
    results, net, st = _search_row(row, ac.CAP)
    want = [_want(row.name, g) for g in range(len(row.fens))]
    for g, (o, vc, rq) in enumerate(want):
        assert not ac.conditions(row, ac.cap_figures(o)), row.names[g]        # the cap binds in the oracle: test_node_cap.py
        assert results[g]["finished"], row.names[g]
        sg._compare(results[g], o, vc, rq)
        assert int(sum(results[g]["n"])) == row.sims
    assert net.calls == sum(o.evals for o, _, _ in want)
    assert st["arena_overflows"] == sum(1 for o, _, _ in want if o.overflow) == len(want)


def test_the_same_searches_in_a_default_arena_match_the_uncapped_oracle():
    """The cap, not the case, makes the difference: the first row with the default arena is the plain oracle's search."""
    row = ac.ROWS[0]
    results, net, st = _search_row(row, 0)
    want = [_want(row.name, g, 0) for g in range(len(row.fens))]
    differ = 0
    for g, (o, vc, rq) in enumerate(want):
        assert not o.overflow
        sg._compare(results[g], o, vc, rq)
        differ += list(vc.values()) != list(_want(row.name, g)[1].values())
    assert differ >= 2                                                       # other root visit counts than under the cap
    assert net.calls == sum(o.evals for o, _, _ in want)
    assert st["arena_overflows"] == 0


def _play_on(e, oracles, boards, results, ply, sims):
    """Play ac.reuse_move of every oracle root in the engine (search_advance) and on the oracle's board."""
    for g, (o, b) in enumerate(zip(oracles, boards)):
        root = o._last_root
        mv = ac.reuse_move(root, ply)
        slot = list(root.children).index(mv)
        assert results[g]["moves"][slot] == mv.uci() and root.children[mv].expanded
        o.note_move_played(mv)
        b.push(mv)
        assert not b.is_game_over()
        e.search_advance(g, slot, sims, True)


@pytest.mark.parametrize("eval_cache", [False, True], ids=["cache_off", "cache_on"])
def test_tree_reuse_across_moves_in_a_full_arena(eval_cache):
    """Three plies from the start position, kiwipete and the 218-move root, the played child's subtree kept: every ply's search
    overflows again (asserted on the oracle), so the engine matches ply by ply only if the re-root counted the kept subtree's
    nodes, cleared the flag and let expansion resume in the other arena half -- and, with the evaluation cache on, left no
    pending-row mark on a refused leaf that the copy would carry into the next search."""
    row = ac.ROWS[0]
    fens = (row.fens[0], row.fens[1], row.fens[3])
    G, L, sims = len(fens), row.leaves, row.sims
    e, _ = sg._engine(G, L, sims, vl_active=True, arena_nodes=ac.CAP, eval_cache=eval_cache)
    net = row.net()
    oracles = [ref.MCTS(ac.oracle_cfg(row), row.net().infer_np, seed=ac.SEED, game=2100 + g) for g in range(G)]
    boards = [ch.Board(f) for f in fens]
    for g, fen in enumerate(fens):
        e.search_begin(g, fen, sims, True, 2100 + g)
    for ply in range(3):
        results = sg._run_engine_search(e, net, G)
        for g, (o, b) in enumerate(zip(oracles, boards)):
            vc, _, rq = o.run(b, num_simulations=sims, ply=ply)
            assert o.overflow and (ply == 0 or 1 < o.next_at_start < ac.CAP), (ply, g)
            assert any(a[5] for a in o.attempts if a[0] == ply), (ply, g)      # expansion resumed after the re-root
            sg._compare(results[g], o, vc, rq)
        if ply < 2:
            _play_on(e, oracles, boards, results, ply, sims)
    st = e.stats()
    e.close()
    assert st["arena_overflows"] == 3 * G
    # (the oracle evaluates a root it takes over once more, mcts.py:359-371; the engine does so only with compat.root_reinfer)
    assert net.calls + st["evals_cached"] == sum(o.evals for o in oracles) - 2 * G
    assert (st["evals_cached"] > 0) == eval_cache


@pytest.mark.parametrize("row", [ac.ROWS[0], ac.ROWS[2], ac.ROWS[6]], ids=[ac.ROWS[0].name, ac.ROWS[2].name, ac.ROWS[6].name])
def test_split_step_with_the_evaluation_cache_in_a_full_arena(row):
    """The evaluation cache changes which leaves go to the network, never the search: with it on, a full arena gives the capped
    oracle's search too -- also where, without virtual loss, a refused leaf is reached again within the pass and shares the first
    sample's row -- and a second search of the same slot from the same root (search_begin again, the cache now warm) equals a
    fresh oracle: nothing of the first search, no pending-row mark of a refused expansion, survived."""
    G = len(row.fens)
    e, _ = sg._engine(G, row.leaves, row.sims, vl_active=row.vl_active, arena_nodes=ac.CAP, eval_cache=True)
    net = row.net()
    want = [_want(row.name, g) for g in range(G)]
    for again in range(2):
        for g, fen in enumerate(row.fens):
            e.search_begin(g, fen, row.sims, True, row.uid0 + g)
        results = sg._run_engine_search(e, net, G)
        for g, (o, vc, rq) in enumerate(want):
            assert results[g]["finished"]
            sg._compare(results[g], o, vc, rq)
    st = e.stats()
    e.close()
    assert st["arena_overflows"] == 2 * G and st["evals_cached"] > 0
    assert net.calls + st["evals_cached"] == 2 * sum(o.evals for o, _, _ in want)


# ---- the analysis engine ----
def _analysis_cfg(row, slots):
    from matrix0_amd import engine as eng
    m = dict(sg.MCTS, inference_batch_size=row.leaves)
    return eng.selfplay_cfg_from_dict({"seed": ac.SEED, "mcts": m, "selfplay": {"num_simulations": row.sims}}, concurrent_games=slots,
                                      virtual_loss_active=row.vl_active, record_games=False, arena_nodes=ac.CAP)


def _analyse(e, step, subs):
    """subs: [(fen, sims, id)] -> {id: result}."""
    for fen, sims, i in subs:
        e.submit(fen, (), sims=sims, id=i)
    got = {}
    for _ in range(100000):
        while (r := e.poll()) is not None:
            got[r["id"]] = r
        if e.pending() == 0:
            break
        step()
    return got


def test_analysis_in_a_full_arena_matches_the_capped_oracle():
    """m0_analysis_* with more simulations than the arena holds (the C ABI allows it; analysis.Analyzer refuses on purpose, hence
    the engine class itself): lines and PVs are those of the capped oracle's tree, a PV stops at a refused leaf whatever its
    visits, `overflow` is the oracle's flag, `sims` what was asked for, and nothing depends on the slot."""
    from matrix0_amd import engine as eng
    rows = [ac.ROWS[0], ac.ROWS[1]]                                         # one engine: same virtual loss, leaves, network
    subs = [(fen, row.sims, row.uid0 + g) for row in rows for g, fen in enumerate(row.fens)]
    want = {row.uid0 + g: _want(row.name, g) for row in rows for g in range(len(row.fens))}
    subs.append((sg.FENS[4], 64, 2200))                                     # and one search that does not fill the arena
    o64 = ref.MCTS(ac.oracle_cfg(rows[0]), rows[0].net().infer_np, seed=ac.SEED, game=2200)
    vc64, _, rq64 = o64.run(ch.Board(sg.FENS[4]), num_simulations=64, ply=0)
    want[2200] = (o64, vc64, rq64)
    assert not o64.overflow
    by_slots = {}
    for slots in (1, 5):
        net = rows[0].net()
        e = eng.AnalysisExtEngine(_analysis_cfg(rows[0], slots), multipv=MULTIPV, pv_len=PV_LEN, dirichlet=True)
        by_slots[slots] = _analyse(e, lambda: e.step(net.infer_np, 8), subs if slots == 1 else subs[::-1])
        st = e.stats()
        e.close()
        assert st["arena_overflows"] == len(subs) - 1
        assert net.calls == sum(o.evals for o, _, _ in want.values())
    assert by_slots[1] == by_slots[5]                                       # every field, floats included
    stopped_at_refused = 0
    for fen, sims, i in subs:
        got, (o, vc, rq) = by_slots[1][i], want[i]
        root = o._last_root
        lines = _oracle_lines(root, MULTIPV, PV_LEN)
        assert got["status"] == "ok" and got["sims"] == sims and got["root_n"] == root.n and got["evals"] == o.evals, i
        assert got["overflow"] == o.overflow, i
        for k in ("move", "policy_index", "visits", "pv"):
            assert [ln[k] for ln in got["lines"]] == [ln[k] for ln in lines], (i, k)
        np.testing.assert_allclose([ln["prior"] for ln in got["lines"]], [ln["prior"] for ln in lines], rtol=0, atol=1e-6)
        np.testing.assert_allclose([ln["q"] for ln in got["lines"]], [ln["q"] for ln in lines], rtol=0, atol=1e-6)
        assert abs(got["root_q"] - rq) < 1e-6, i
        refused = {id(a[2]) for a in o.attempts if not a[5]} - {id(a[2]) for a in o.attempts if a[5]}
        for ln in lines:
            node = root
            for u in ln["pv"]:
                node = node.children[ch.Move.from_uci(u)]
            stopped_at_refused += id(node) in refused and node.n > 1 and len(ln["pv"]) < PV_LEN
    assert stopped_at_refused > 0


def test_analysis_on_the_engines_network_in_a_full_arena_fused_equals_split():
    """AnalysisEngine (m0_analysis_step, the network inside) against AnalysisExtEngine fed by the same network: bit for bit, as in
    tests/test_analysis_gpu.py, with searches that overflow."""
    from matrix0_amd import engine as eng
    from matrix0_amd.backend import M0Backend
    row = ac.ROWS[0]
    subs = [(fen, row.sims, row.uid0 + g) for g, fen in enumerate(row.fens)]
    be = M0Backend.from_state_dict(tp.NET, net_ref.random_state_dict(tp.NET, seed=7))
    e = eng.AnalysisEngine(be, _analysis_cfg(row, 3), multipv=MULTIPV, pv_len=PV_LEN, dirichlet=True)
    fused = _analyse(e, lambda: e.step(8), subs)
    st_f = e.stats()
    e.close()
    e = eng.AnalysisExtEngine(_analysis_cfg(row, 3), multipv=MULTIPV, pv_len=PV_LEN, dirichlet=True)
    split = _analyse(e, lambda: e.step(be.infer_np, 8), subs)
    st_s = e.stats()
    e.close()
    be.close()
    assert fused == split and sorted(fused) == [i for _, _, i in subs]
    assert all(r["sims"] == row.sims and sum(ln["visits"] for ln in r["lines"]) <= row.sims for r in fused.values())
    overflowed = sum(r["overflow"] for r in fused.values())                 # (another network than the case table's)
    assert st_f["arena_overflows"] == st_s["arena_overflows"] == overflowed >= 2 and st_f["evals"] == st_s["evals"]


# ---- whole games ----
GAME_CFG = dict(tp.CFG, selfplay=dict(tp.CFG["selfplay"], num_simulations=400, max_game_len=6))


def _fused_games(be, cfg, **kw):
    from matrix0_amd import engine as eng
    e = eng.SelfplayEngine(be, eng.selfplay_cfg_from_dict(cfg, **kw))
    games = {}
    for _ in range(20000):
        e.step(4)
        while (r := e.poll()) is not None:
            games[r["game_index"]] = r
        if not e.running():
            break
    st = e.stats()
    e.close()
    return games, st


def test_fused_step_equals_split_step_in_a_full_arena():
    from matrix0_amd import engine as eng
    from matrix0_amd.backend import M0Backend
    be = M0Backend.from_state_dict(tp.NET, net_ref.random_state_dict(tp.NET, seed=7))
    kw = dict(concurrent_games=3, total_games=3, arena_nodes=ac.CAP)
    fused, st_f = _fused_games(be, GAME_CFG, **kw)
    again, st_a = _fused_games(be, GAME_CFG, **kw)
    e = eng.SelfplayEngine(be, eng.selfplay_cfg_from_dict(GAME_CFG, **kw))
    split = {}
    for _ in range(80000):
        planes = e.ext_select()
        lg, vv = be.infer_np(planes) if planes.shape[0] else (np.zeros((0, 4672), np.float32), np.zeros((0,), np.float32))
        e.ext_expand(lg, vv)
        while (r := e.poll()) is not None:
            split[r["game_index"]] = r
        if not e.running():
            break
    st_s = e.stats()
    e.close()
    be.close()
    assert sorted(fused) == sorted(again) == sorted(split) == [0, 1, 2]
    for k in ("evals", "sims", "plies", "games_finished", "steps", "arena_overflows"):
        assert st_f[k] == st_s[k] == st_a[k], k
    assert st_f["arena_overflows"] > 0
    for i in range(3):
        tp._records_equal(fused[i], split[i], ("split", i))
        tp._records_equal(fused[i], again[i], ("again", i))


@pytest.mark.parametrize("mode", ["tree_reuse_vl", "fresh_tree_no_vl"])
def test_games_in_a_full_arena_are_identical_with_and_without_the_cache(mode):
    """tests/test_eval_cache_gpu.py's contract where the arena is full.  Without virtual loss and two leaves per pass the second
    leaf of a pass is very often the first again: with the cache off both are evaluated and both try to expand, with it on the
    second shares the first one's row -- and has to try again after a refusal, or the entropy-noise stream of the two runs parts."""
    from matrix0_amd.backend import M0Backend
    be = M0Backend.from_state_dict(ecg.NET, net_ref.random_state_dict(ecg.NET, seed=9))
    cfg = dict(ecg.CFG, selfplay=dict(ecg.CFG["selfplay"], num_simulations=400, max_game_len=6))
    kw = dict(arena_nodes=ac.CAP)
    if mode == "fresh_tree_no_vl":
        kw.update(virtual_loss_active=False, compat={"fresh_tree_per_move": True}, leaves_per_step=2)
    off, st_off = ecg._play(be, False, cfg, **kw)
    on, st_on = ecg._play(be, True, cfg, **kw)
    be.close()
    print(f"full arena [{mode}]: overflows {int(st_off['arena_overflows'])} off / {int(st_on['arena_overflows'])} on, "
          f"{int(st_on['evals_cached'])} of {int(st_off['evals'])} evaluations from the cache")
    assert sorted(off) == sorted(on) == list(range(8))
    for i in range(8):
        a, b = off[i], on[i]
        assert a["played"] == b["played"] and a["result"] == b["result"], i
        for k in ("pi", "z", "s", "legal_mask", "search_values"):
            assert np.array_equal(a[k], b[k]), (i, k)
    assert st_off["evals_cached"] == 0 and st_on["evals_cached"] > 0
    assert st_on["sims"] == st_off["sims"] and st_on["plies"] == st_off["plies"]
    assert st_on["evals"] + st_on["evals_cached"] == st_off["evals"]
    assert st_off["arena_overflows"] > 0 and st_on["arena_overflows"] == st_off["arena_overflows"]
