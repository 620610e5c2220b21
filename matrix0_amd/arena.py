"""Evaluation matches between two networks on one MI355X: the device-resident counterpart of
azchess/arena.py.  `play_match` keeps the reference's call shape and return value (the summed score of A);
all games of the match are played concurrently by one engine (m0_arena_create), each search evaluated by the network
of the side to move.

Semantics kept from the reference (file:line = azchess/arena.py): game i gives A the white pieces when i is even (:66);
a game runs while `not board.is_game_over(claim_draw=True)` and fewer than `max_moves` plies were played, with the draw
adjudication test of draw.py before every search (:67-72); the move is sampled from softmax(log(visits+1e-8)/temp) for
the first `temp_plies` plies when temp > 1e-3, otherwise the most visited move (:73-106); unfinished games score 1/2
(:110-124); evaluation searches use no Dirichlet noise unless `eval.dirichlet_frac` says so and no entropy noise
(:365-381); Wilson interval (:272-278), Elo update (elo.py:10-22), PGN files game_NNNN.pgn (:281-303).
Search structure: by default every move starts a fresh tree.  The reference keeps one MCTS object -- hence one transposition
table -- per side for the whole game (:157-158): `engine.compat.tt_merge: true` gives the match engine exactly that (one
device table per side and game, roots looked up in it, later searches merging into the nodes earlier ones left there; size
`engine.arena_nodes` for all nodes a side creates in a game).  Both modes replay the reference's own arena games move for move
(tests/golden/ref_arena.json.gz, tests/test_golden_selfplay_gpu.py).

Two opt-in additions the reference has no code for.  `engine.arena_eval_cache: true` (entries: `engine.eval_cache_entries`)
gives every network an evaluation cache per game: a side's fresh tree re-expands what its own search of two plies earlier
evaluated, and those leaves are served from the cache instead of the network -- the same games, fewer evaluations
(`last_match_stats["evals_cached"]`).  `eval.openings_pgn` (the key of the reference's config.yaml, which nothing there reads) or
the `openings=` argument starts the games from an opening book, paired by colour: games 2k and 2k+1 share one book position, so
each opening is played once with A as White and once with B.  Without a book every game starts from the initial position, and
with no temperature and no noise a match is then two distinct games played over and over.

A third: `engine.tablebase: {max_pieces, cache, in_search: true}` (matrix0_amd/tablebase.py) or the `tablebase=` argument puts
the generated endgame tables into the match: the searches of both sides take the exact value of every leaf found in them, and
a game ends with the table's verdict as soon as the position after a move is inside them
(`last_match_stats["tb_adjudications"]`, `["tb_leaves"]`).  Without `in_search` the key is ignored here, as before."""
from __future__ import annotations

import json
import os
import time
import warnings
from datetime import datetime
from typing import Dict, List, Optional, Tuple

from . import engine as eng
from .pgn import save_pgn

K_DEFAULT = 20.0


def wilson_interval(p: float, n: int, z: float = 1.96) -> Tuple[float, float]:
    if n == 0:
        return 0.0, 0.0
    denom = 1 + z * z / n
    center = (p + (z * z) / (2 * n)) / denom
    half = (z * ((p * (1 - p) / n) + (z * z) / (4 * n * n)) ** 0.5) / denom
    return max(0.0, center - half), min(1.0, center + half)


def expected_score(ra: float, rb: float) -> float:
    return 1.0 / (1.0 + 10.0 ** ((rb - ra) / 400.0))


def update_elo(ra: float, rb: float, sa: float, k: float = K_DEFAULT) -> Tuple[float, float]:
    delta = k * (sa - expected_score(ra, rb))
    return ra + delta, rb - delta


def result_string(z_white: float, finished: bool) -> str:
    if not finished or z_white == 0.0:
        return "1/2-1/2"
    return "1-0" if z_white > 0 else "0-1"


def game_score(result: str, a_is_white: bool) -> float:
    if result == "1-0":
        return 1.0 if a_is_white else 0.0
    if result == "0-1":
        return 0.0 if a_is_white else 1.0
    return 0.5


def arena_cfg_from_dict(cfg: dict, *, games: int, num_sims: int, max_moves: int, temp: float, temp_plies: int,
                        concurrent_games: int, leaves_per_step: Optional[int], seed: Optional[int]) -> eng.SelfplayCfg:
    """MCTS settings as play_match builds them (arena.py:361-381): config.yaml's mcts section with num_simulations,
    eval.dirichlet_frac (default 0), selfplay.selection_jitter, entropy noise off."""
    m = dict(cfg.get("mcts", {}) or {})
    sp = dict(cfg.get("selfplay", {}) or {})
    ev = dict(cfg.get("eval", {}) or {})
    m.update({"dirichlet_frac": float(ev.get("dirichlet_frac", 0.0)), "selection_jitter": float(sp.get("selection_jitter", 0.0)),
              "enable_entropy_noise": False})
    draw = dict(cfg.get("draw", {}) or {})
    ecfg = dict(cfg.get("engine", {}) or {})
    cfg2 = {"seed": cfg.get("seed", 1234), "mcts": m, "draw": draw, "engine": {"compat": dict(ecfg.get("compat", {}) or {})},
            "selfplay": {"num_simulations": int(num_sims), "max_game_len": int(max_moves), "opening_random_plies": 0,
                         "resign_threshold": -2.0, "min_resign_plies": 10 ** 9}}
    c = eng.selfplay_cfg_from_dict(cfg2, concurrent_games=concurrent_games, total_games=games, seed=seed,
                                   leaves_per_step=leaves_per_step, virtual_loss_active=bool(ecfg.get("virtual_loss_active", True)),
                                   record_games=False, arena_nodes=int(ecfg.get("arena_nodes", 0) or 0))
    c.arena_temp = float(temp)
    c.arena_temp_plies = int(temp_plies)
    # one evaluation cache per network and game (`engine.eval_cache` is the self-play switch; a match engine ignores it)
    c.arena_eval_cache = int(bool(ecfg.get("arena_eval_cache", False)))
    c.eval_cache_entries = int(ecfg.get("eval_cache_entries", 0) or 0)
    return c


def match_openings(cfg: dict, openings: Optional[List[str]] = None) -> List[str]:
    """The opening book of a match as FEN strings: the `openings` argument, else the PGN file `eval.openings_pgn` names (read by
    pgn_book.load_opening_book), else [] = every game starts from the initial position."""
    if openings is not None:
        return [str(f) for f in openings]
    path = (cfg.get("eval", {}) or {}).get("openings_pgn")
    if not path:
        return []
    from .pgn_book import load_opening_book
    book = load_opening_book(str(path))
    if not book:
        warnings.warn(f"eval.openings_pgn: no opening positions in {path!r}; the games start from the initial position")
    return book


last_match_stats: Dict[str, float] = {}


def play_match(backend_a, backend_b, games: int, cfg: dict, seed: Optional[int] = None, pgn_out: Optional[str] = None,
               pgn_sample: int = 0, num_sims: int = 500, max_moves_override: Optional[int] = None, temp: float = 0.0,
               temp_plies: int = 0, concurrent_games: Optional[int] = None, leaves_per_step: Optional[int] = 16,
               elo_book: Optional[str] = None, log_dir: Optional[str] = None, progress=None,
               openings: Optional[List[str]] = None, tablebase=None) -> float:
    """A vs B over `games` games; returns the summed score of A (1 / 0.5 / 0 per game), as arena.play_match does.
    `backend_a` / `backend_b` are M0Backend objects on the same device (the reference takes checkpoint paths:
    M0Backend.from_checkpoint).  `openings` (FEN strings) or `eval.openings_pgn` in `cfg`: the games start from book positions,
    games 2k and 2k+1 from the same one; `max_moves` then counts the plies played from there.  Details of the last match
    (W/L/D, win rate, Wilson interval, Elo, evaluations made and served from the cache, the records with their `start_fen`) are
    left in `last_match_stats`.  `tablebase` (a Tablebase) or `engine.tablebase` with `in_search: true` in `cfg`: the endgame tables
    are probed inside the searches and end a game that enters them, with their result.  `engine.proof_search: true` in `cfg`: the
    proof search (SelfplayEngine.set_proof) -- a proven mate is played, a move that is proven lost is not, a search ends once
    its root is proven."""
    global last_match_stats
    if games <= 0:
        return 0.0
    ev = dict(cfg.get("eval", {}) or {})
    max_moves = int(max_moves_override) if max_moves_override is not None else int(ev.get("max_moves", 300))
    conc = int(concurrent_games or min(games, 256))
    ecfg = dict(cfg.get("engine", {}) or {})
    if bool((ecfg.get("compat", {}) or {}).get("tt_merge", False)) and not int(ecfg.get("arena_nodes", 0) or 0):
        # per-side tables for the whole game: nothing is compacted, so a side's arena half must hold every node it creates in the
        # game (~40 per simulation and search).  Size it, and keep the resident games within ~96 GB of node storage.
        nodes = int(min(8_000_000, max(65536, num_sims * 40 * (max_moves // 2 + 2))))
        tcap = 1024
        while tcap < 2 * nodes:                                        # alloc_position_tables rounds a table up to a power of two
            tcap <<= 1
        per_game = 2 * nodes * 46 + 2 * tcap * 12                      # two halves of SoA nodes + two tables (8-byte key + 4-byte node)
        conc = max(1, min(conc, int(96e9 // per_game)))
        cfg = dict(cfg, engine=dict(ecfg, arena_nodes=nodes))
    c = arena_cfg_from_dict(cfg, games=games, num_sims=num_sims, max_moves=max_moves, temp=temp, temp_plies=temp_plies,
                            concurrent_games=min(conc, games), leaves_per_step=leaves_per_step, seed=seed)
    book = match_openings(cfg, openings)
    c.arena_paired_openings = 1 if book else 0
    from . import tablebase as tbm
    tb_cfg = tbm.tablebase_cfg(cfg)
    tb, tb_limit, tb_owned = tablebase, 4, False
    if tb is None and tb_cfg is not None and tb_cfg.get("in_search", False):
        tb = tbm.Tablebase.cached(tb_cfg["cache"], tb_cfg["max_pieces"], int(ecfg.get("device_index", 0) or 0))
        tb_owned = True
    if tb is not None and tb_cfg is not None:
        tb_limit = tbm.probe_limit(cfg)
    e = eng.ArenaEngine(backend_a, backend_b, c)
    tb_stats = {"tb_adjudications": 0.0, "tb_leaves": 0.0}
    score = 0.0
    a_wins = b_wins = draws = 0
    done: List[dict] = []
    t0 = time.perf_counter()
    try:
        if book:
            e.set_openings(book)
        if tb is not None:
            e.set_search_tablebase(tb, tb_limit)
        if bool(ecfg.get("proof_search", False)):
            e.set_proof()                       # exact wins, losses and draws are backed up the tree; the engine plays the search's pick
        while e.running():
            e.step(8)
            while (r := e.poll()) is not None:
                a_white = (r["game_index"] % 2 == 0)
                # result from White's point of view; 0 also for games cut at max_moves / adjudicated (scored 1/2)
                res = result_string(float(r["result"]), True)
                sc = game_score(res, a_white)
                score += sc
                if sc == 1.0:
                    a_wins += 1
                elif sc == 0.0:
                    b_wins += 1
                else:
                    draws += 1
                r["result_str"] = res
                r["score_a"] = sc
                done.append(r)
                if pgn_out and (pgn_sample <= 0 or len(done) <= pgn_sample):
                    save_pgn(r["played_raw"], res, {"Event": "Matrix0 arena", "Round": r["game_index"] + 1,
                                                    "White": "A" if a_white else "B", "Black": "B" if a_white else "A",
                                                    "Date": datetime.now().strftime("%Y.%m.%d")}, pgn_out, r["game_index"],
                             start_fen=r.get("start_fen"))
                if progress is not None:
                    progress(len(done), games, a_wins, b_wins, draws)
    finally:
        st = e.stats()
        if tb is not None:
            tb_stats = {"tb_adjudications": float(e.tb_adjudications()), "tb_leaves": float(e.tb_leaves())}
        e.close()                      # the engine first: the tables outlive it
        if tb_owned:
            tb.close()
    win_rate = score / float(max(1, games))
    lo, hi = wilson_interval(win_rate, games)
    stats = {"games": games, "a_wins": a_wins, "b_wins": b_wins, "draws": draws, "score": score, "win_rate": win_rate,
             "wilson_low": lo, "wilson_high": hi, "seconds": time.perf_counter() - t0, "evals": float(st["evals"]),
             "evals_cached": float(st["evals_cached"]), "plies": float(st["plies"]), "records": done, **tb_stats}
    if elo_book:
        book = {"best": 1500.0, "enhanced_best": 1500.0, "candidate": 1500.0, "baseline": 1500.0, "history": []}
        if os.path.exists(elo_book):
            try:
                book = json.loads(open(elo_book).read())
            except Exception:
                pass
        ra, rb = update_elo(float(book.get("candidate", 1500.0)), float(book.get("best", 1500.0)), win_rate)
        book["candidate"], book["best"] = ra, rb
        book.setdefault("history", []).append({"win_rate": win_rate, "games": games, "timestamp": int(time.time())})
        os.makedirs(os.path.dirname(elo_book) or ".", exist_ok=True)
        open(elo_book, "w").write(json.dumps(book, indent=2))
        stats["elo_candidate"], stats["elo_best"] = ra, rb
    if log_dir:
        os.makedirs(log_dir, exist_ok=True)
        with open(os.path.join(log_dir, "eval_summary.jsonl"), "a") as f:
            f.write(json.dumps({"type": "eval_summary", "games": int(games), "a_wins": a_wins, "b_wins": b_wins,
                                "draws": draws, "win_rate": float(win_rate), "timestamp": int(time.time())}) + "\n")
    last_match_stats = stats
    return score
