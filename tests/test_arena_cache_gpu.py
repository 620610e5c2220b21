"""`engine.arena_eval_cache`: a match engine keeps one evaluation cache per network and game (csrc/tree.h EvalCache with
sides = 2, csrc/eval_cache.h).  Every move of a match starts a fresh tree, so a side's new root and everything below it was
evaluated by that same network two plies earlier; with the switch on those leaves are expanded from the cache.  The 320-wide
forward is bitwise batch invariant, so a cached answer is the answer a fresh evaluation would give: the games must be the same
bit for bit, every evaluation of the off-run is an evaluation or a hit of the on-run, and nothing network A said may ever reach
a search of network B."""
import numpy as np
import pytest

from oracle import chess_py as ch
from oracle import net_ref
from tests.golden_ref import load_json, uci as _uci
from tests.hash_net import HashNet

pytestmark = pytest.mark.gpu

WIDE = dict(planes=19, channels=320, blocks=2, attention_heads=20, policy_size=4672, norm="group", activation="silu",
            preact=True, policy_factor_rank=128, self_supervised=False)
CFG = {"seed": 7,
       "mcts": {"cpuct": 2.5, "cpuct_start": 3.0, "cpuct_end": 2.0, "cpuct_plies": 40, "dirichlet_plies": 30,
                "dirichlet_frac": 0.25, "selection_jitter": 0.0, "fpu_reduction": 0.1, "draw_penalty": -0.05,
                "legal_softmax": True, "inference_batch_size": 8, "playout_random_frac": 0.0},
       "selfplay": {"selection_jitter": 0.0},
       "eval": {"max_moves": 40},
       "draw": {"min_plies": 30, "window": 8, "min_unique": 4, "halfmove_cap": 100}}


def _wide_backends(bias_b=None):
    from matrix0_amd.backend import M0Backend
    sd_a = net_ref.random_state_dict(WIDE, seed=1)
    sd_b = net_ref.random_state_dict(WIDE, seed=2)
    for idx in bias_b or ():
        sd_b["policy_fc2.bias"][idx] += 100.0          # the logit scale of these weights is 0.2: 20 logits above the rest
    return M0Backend.from_state_dict(WIDE, sd_a), M0Backend.from_state_dict(WIDE, sd_b)


def _match(a, b, cfg, *, games, sims, max_moves, temp, temp_plies, conc, L, seed, arena_cache=None, eval_cache=0):
    """One match on the match engine itself; {game index: record}, engine statistics."""
    from matrix0_amd import arena, engine as eng
    c = arena.arena_cfg_from_dict(cfg, games=games, num_sims=sims, max_moves=max_moves, temp=temp, temp_plies=temp_plies,
                                  concurrent_games=conc, leaves_per_step=L, seed=seed)
    if arena_cache is not None:
        c.arena_eval_cache = int(arena_cache)
    c.eval_cache = int(eval_cache)
    e = eng.ArenaEngine(a, b, c)
    recs = {}
    while e.running():
        e.step(8)
        while (r := e.poll()) is not None:
            recs[r["game_index"]] = r
    st = e.stats()
    e.close()
    return recs, st


def _same_games(off, on):
    assert sorted(off) == sorted(on)
    for i in sorted(off):
        x, y = off[i], on[i]
        assert x["played"] == y["played"] and x["result"] == y["result"], i
        assert np.array_equal(x["search_values"], y["search_values"]), i


def test_match_is_identical_with_the_per_side_cache_and_evaluations_add_up():
    a, b = _wide_backends()
    kw = dict(games=6, sims=64, max_moves=18, temp=1.0, temp_plies=6, conc=4, L=16, seed=11)
    off, st_off = _match(a, b, CFG, arena_cache=0, **kw)
    on, st_on = _match(a, b, CFG, arena_cache=1, **kw)
    a.close(); b.close()
    assert sorted(off) == list(range(6))
    _same_games(off, on)
    assert st_on["sims"] == st_off["sims"] and st_on["plies"] == st_off["plies"]
    print(f"arena eval cache: {int(st_on['evals_cached'])} of {int(st_off['evals'])} leaf evaluations served "
          f"({100.0 * st_on['evals_cached'] / st_off['evals']:.1f} %); evaluations made {int(st_on['evals'])}")
    assert st_on["evals"] + st_on["evals_cached"] == st_off["evals"]
    assert st_off["evals_cached"] == 0 and st_on["evals_cached"] > 0


def test_the_two_networks_do_not_share_entries():
    """B's policy head is rigged to open a2a3; A's is not.  One game slot plays all four games, so both networks' caches see
    the same positions over and over (the start position's subtree in every game): with the cache on B still opens a2a3 in
    the odd games, and every game -- A's even ones in particular -- is the game of the cache-off run, values included."""
    start = ch.Board()
    i_w = ch.move_to_index(start, ch.Move.from_uci("a2a3"))
    a, b = _wide_backends(bias_b=[i_w])
    kw = dict(games=4, sims=32, max_moves=6, temp=0.0, temp_plies=0, conc=1, L=8, seed=3)
    off, st_off = _match(a, b, CFG, arena_cache=0, **kw)
    on, st_on = _match(a, b, CFG, arena_cache=1, **kw)
    a.close(); b.close()
    for i in (1, 3):
        assert off[i]["played"][0] == "a2a3" and on[i]["played"][0] == "a2a3", i     # B is White in the odd games
    for i in (0, 2):
        assert on[i]["played"][0] != "a2a3" and on[i]["played"] == off[i]["played"], i
    _same_games(off, on)
    assert st_on["evals_cached"] > 0 and st_on["evals"] + st_on["evals_cached"] == st_off["evals"]


ARENA = load_json("ref_arena.json.gz")
TABLE_OFF = [i for i, g in enumerate(ARENA["games"]) if g["tt"] == "off"]


def _replay_golden(g, cache):
    """The reference's arena game through m0_arena_create_ext; the record, the rows each evaluator saw, the hits per network."""
    from matrix0_amd import engine as eng
    cfg_dict = {"seed": ARENA["seed"], "mcts": dict(g["mcts"]), "draw": dict(g["draw"]),
                "selfplay": {"num_simulations": g["sims"], "max_game_len": g["max_moves"], "opening_random_plies": 0}}
    cfg = eng.selfplay_cfg_from_dict(cfg_dict, concurrent_games=1, total_games=1, first_game_index=g["uid"],
                                     virtual_loss_active=False, record_games=True)
    cfg.arena_temp, cfg.arena_temp_plies = float(g["temp"]), int(g["temp_plies"])
    cfg.arena_eval_cache = int(cache)
    e = eng.ArenaExtEngine(cfg)
    na, nb = HashNet(**g["net_a"]), HashNet(**g["net_b"])
    z0 = (np.zeros((0, 4672), np.float32), np.zeros((0,), np.float32))
    hits, seen = [0, 0], 0
    rec = None
    for _ in range(100000):
        if not e.running():
            break
        # one game from the initial position: White searches at even plies, and A is White when the game index is even
        side = 0 if (int(e.stats()["plies"]) % 2 == 0) == (g["uid"] % 2 == 0) else 1
        pa, pb = e.arena_ext_select()
        assert (pb if side == 0 else pa).shape[0] == 0, "rows for the network that does not search"
        la, va = na.infer_np(pa) if pa.shape[0] else z0
        lb, vb = nb.infer_np(pb) if pb.shape[0] else z0
        e.arena_ext_expand(la, va, lb, vb)
        now = int(e.stats()["evals_cached"])
        hits[side] += now - seen
        seen = now
        rec = rec or e.poll()
    rec = rec or e.poll()
    st = e.stats()
    e.close()
    assert rec is not None and rec["game_index"] == g["uid"]
    return rec, (na.calls, nb.calls), hits, st


@pytest.mark.parametrize("gi", [i for i in TABLE_OFF if ARENA["games"][i]["uid"] in (0, 2, 4)])
def test_golden_arena_games_replay_with_the_cache_on_and_off(gi):
    g = ARENA["games"][gi]
    want = [_uci(t["moves"][k]) for t, k in zip(g["trace"], g["chosen"])]
    for cache in (0, 1):
        rec, calls, hits, st = _replay_golden(g, cache)
        assert rec["moves"] == g["plies"] and rec["played"] == want, cache
        for t, w in enumerate(g["trace"]):
            tot = float(sum(w["visits"]))
            pi = np.zeros(4672, np.float32)
            for i, n in zip(w["idx"], w["visits"]):
                pi[i] = np.float32(n / tot)
            assert np.array_equal(rec["pi"][t], pi), (cache, t)
            assert abs(float(rec["search_values"][t]) - w["root_q"]) < 1e-6, (cache, t)
        print(f"golden arena game uid {g['uid']} cache {cache}: rows {calls}, hits {hits}, golden ({g['evals_a']}, {g['evals_b']})")
        assert (calls[0] + hits[0], calls[1] + hits[1]) == (g["evals_a"], g["evals_b"]), cache
        assert sum(hits) == st["evals_cached"] and st["evals"] == sum(calls)
        assert (sum(hits) > 0) == bool(cache)


@pytest.mark.parametrize("mode", ["tt_merge", "full_softmax"])
def test_switch_is_ignored_where_the_payload_cannot_serve_the_expansion(mode):
    a, b = _wide_backends()
    cfg = {k: (dict(v) if isinstance(v, dict) else v) for k, v in CFG.items()}
    if mode == "tt_merge":
        cfg["engine"] = {"compat": {"tt_merge": True}, "arena_nodes": 65536}
    else:
        cfg["mcts"] = dict(cfg["mcts"], legal_softmax=False)
    kw = dict(games=2, sims=32, max_moves=8, temp=1.0, temp_plies=4, conc=2, L=8, seed=21)
    off, st_off = _match(a, b, cfg, arena_cache=0, **kw)
    on, st_on = _match(a, b, cfg, arena_cache=1, **kw)
    a.close(); b.close()
    assert st_on["evals_cached"] == 0 and st_on["evals"] == st_off["evals"]
    _same_games(off, on)


def test_eval_cache_alone_is_still_ignored_by_a_match_engine():
    a, b = _wide_backends()
    kw = dict(games=2, sims=32, max_moves=8, temp=1.0, temp_plies=4, conc=2, L=8, seed=9)
    off, st_off = _match(a, b, CFG, **kw)
    on, st_on = _match(a, b, CFG, eval_cache=1, **kw)
    a.close(); b.close()
    assert st_on["evals_cached"] == 0 and st_on["evals"] == st_off["evals"]
    _same_games(off, on)


def test_play_match_reports_the_hits():
    """`engine.arena_eval_cache` through play_match: same score and games, `evals_cached` in last_match_stats."""
    from matrix0_amd import arena
    a, b = _wide_backends()
    kw = dict(seed=5, num_sims=32, temp=1.0, temp_plies=4, max_moves_override=10, concurrent_games=2, leaves_per_step=8)
    s_off = arena.play_match(a, b, 2, CFG, **kw)
    off = arena.last_match_stats
    s_on = arena.play_match(a, b, 2, dict(CFG, engine={"arena_eval_cache": True, "eval_cache_entries": 4096}), **kw)
    on = arena.last_match_stats
    a.close(); b.close()
    assert s_on == s_off and off["evals_cached"] == 0 and on["evals_cached"] > 0
    assert on["evals"] + on["evals_cached"] == off["evals"]
    assert {r["game_index"]: r["played"] for r in on["records"]} == {r["game_index"]: r["played"] for r in off["records"]}
