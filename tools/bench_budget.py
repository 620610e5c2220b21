#!/usr/bin/env python3
"""Self-play with and without the budget mix (mcts.budget, include/m0_budget.h) on bench.py's workload: random-weight R24-320,
256 concurrent games, 800 simulations per full search at 96 leaves per tree and pass.  Mode off against mode on at the defaults
(full_prob 0.25, 100 fast simulations, forced_k 2, pruned targets), alternating twice in one process so that a drift of the
clocks shows as a difference between the two runs of one setting.

With the mode on the searches of a launch no longer end together -- a fast search takes 2 passes, a full one 9 -- so the timed
region is a number of passes, not of plies.  Per run one JSON line, also appended to profiles/budget.log:
  searched_plies_per_s     plies searched and played per second: what brings a game to its result
  plies_per_game_slot      searched plies per resident game in the timed region (the game-equivalents the region covered are
                           this over the plies of a game)
  training_rows_per_s      plies that become training rows per second: every ply with the mode off, the full ones with it on
  ms_tree_per_pass         select + expand per pass: the PUCT instantiation of select_kernel with the mode off, the forced one
                           with it on
  the four counters of m0_selfplay_budget_stats over the region (mode on)

usage: bench_budget.py [passes=180] [warmup_passes=27]"""
import json, os, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import torch
from matrix0_amd.backend import M0Backend
from matrix0_amd.weights import random_state_dict
from matrix0_amd import engine as eng
import bench

passes = int(sys.argv[1]) if len(sys.argv) > 1 else 180
warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 27
GAMES, SIMS, LEAVES = 256, 800, 96
LOG = os.path.join(ROOT, "profiles", "budget.log")
be = M0Backend.from_state_dict(bench.R24_320, random_state_dict(bench.R24_320, seed=0, varied=True))

for rep in range(2):
    for mode in ("off", "on"):
        cfg = json.loads(json.dumps(bench.SELFPLAY_CFG))
        cfg["selfplay"]["num_simulations"] = SIMS
        if mode == "on":
            cfg["mcts"]["budget"] = {"enabled": True}
        e = eng.SelfplayEngine(be, eng.selfplay_cfg_from_dict(cfg, concurrent_games=GAMES, total_games=0, leaves_per_step=LEAVES,
                                                              virtual_loss_active=True, record_games=False, eval_cache=True))
        b = eng.budget_cfg_from_dict(cfg)
        if b is not None:
            e.set_budget(b)
        e.step(warmup)
        torch.cuda.synchronize()
        s0, b0, t0 = e.stats(), (e.budget_stats() if b is not None else None), time.perf_counter()
        e.step(passes)
        torch.cuda.synchronize()
        dt, s1, b1 = time.perf_counter() - t0, e.stats(), (e.budget_stats() if b is not None else None)
        e.close()
        d = {k: s1[k] - s0[k] for k in ("plies", "evals", "steps", "sims", "ms_tree", "ms_net", "games_finished")}
        counters = {k: b1[k] - b0[k] for k in b1} if b is not None else None
        # a ply counted in the region was armed before it was played: the searches armed in the region stand in for the rows
        rows = d["plies"] if counters is None else d["plies"] * counters["full_searches"] / max(
            1, counters["full_searches"] + counters["fast_searches"])
        line = json.dumps({"budget": mode, "run": rep, "games": GAMES, "sims": SIMS, "leaves": LEAVES, "passes": int(d["steps"]),
                           "seconds": round(dt, 3), "searched_plies_per_s": round(d["plies"] / dt, 1),
                           "plies_per_game_slot": round(d["plies"] / GAMES, 2),
                           "training_rows_per_s": round(rows / dt, 1), "evals_per_s": round(d["evals"] / dt),
                           "sims_per_ply": round(d["sims"] / max(1, d["plies"]), 1),
                           "ms_tree_per_pass": round(d["ms_tree"] / max(1, d["steps"]), 3),
                           "ms_net_per_pass": round(d["ms_net"] / max(1, d["steps"]), 3), "counters": counters})
        print(line, flush=True)
        os.makedirs(os.path.dirname(LOG), exist_ok=True)
        with open(LOG, "a") as f:
            f.write(line + "\n")
be.close()
