#!/usr/bin/env python3
"""Throughput of the evaluation-match engine at the benchmark size: two R24-320 networks, 256 concurrent games,
800 simulations per move, games cut after a few plies.  The same match is timed with the per-side evaluation cache
(`engine.arena_eval_cache`) off and on, alternating, `repeats` times each: one JSON line per run.  The off-run is the engine's
default.  The share of evaluations the cache serves grows with the ply (a side's first search of a game finds its cache
empty), so compare runs of the same length.

usage: bench_arena.py [plies_per_game=4] [repeats=1]"""
import json, os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from oracle import net_ref
from matrix0_amd.backend import M0Backend
from matrix0_amd import arena
import bench

plies = int(sys.argv[1]) if len(sys.argv) > 1 else 4
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 1
a = M0Backend.from_state_dict(bench.R24_320, net_ref.random_state_dict(bench.R24_320, seed=0))
b = M0Backend.from_state_dict(bench.R24_320, net_ref.random_state_dict(bench.R24_320, seed=1))
for rep in range(repeats):
    for cache in (False, True):
        cfg = dict(bench.SELFPLAY_CFG, eval={"max_moves": plies}, engine={"arena_eval_cache": cache})
        t0 = time.perf_counter()
        score = arena.play_match(a, b, 256, cfg, seed=1, num_sims=800, temp=1.0, temp_plies=30, concurrent_games=256, leaves_per_step=16)
        dt = time.perf_counter() - t0
        st = arena.last_match_stats
        leaves = st["evals"] + st["evals_cached"]
        print(json.dumps({"arena_eval_cache": int(cache), "run": rep, "games": 256, "plies_per_game": plies, "seconds": round(dt, 2),
                          "evals": st["evals"], "evals_cached": st["evals_cached"],
                          "served_share": round(st["evals_cached"] / max(1.0, leaves), 4), "evals_per_s": round(st["evals"] / dt),
                          "leaves_per_s": round(leaves / dt), "searched_plies_per_s": round(st["plies"] / dt, 1), "score_a": score,
                          "games_per_s_at_100_plies": round(st["plies"] / dt / 100.0, 3)}), flush=True)
a.close(); b.close()
