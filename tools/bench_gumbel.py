#!/usr/bin/env python3
"""Self-play at small simulation budgets: the Gumbel root search (mcts.gumbel, include/m0_gumbel.h) beside the PUCT root at the
same number of simulations per move.  Random-weight R24-320, max_considered = 16, n in {16, 32, 64} simulations and 256 or
1024 concurrent games, one pass of at most n leaves per game (leaves_per_step = n for both roots).  The Gumbel root's passes
end at the phase boundaries of the halving schedule, so its batches are smaller than PUCT's: whether they still fill the chip
is what the rows-per-forward and evaluations/s columns answer.

Per setting one JSON line, also appended to profiles/gumbel.log: searched plies/s, evaluations/s, rows per forward and passes
per search over a timed region of `plies` searched plies per resident game after `warmup` of them.

usage: bench_gumbel.py [plies=30] [warmup=3]"""
import json, os, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import torch
from matrix0_amd.backend import M0Backend
from matrix0_amd.weights import random_state_dict
from matrix0_amd import engine as eng
import bench

plies = int(sys.argv[1]) if len(sys.argv) > 1 else 30
warmup = int(sys.argv[2]) if len(sys.argv) > 2 else 3
LOG = os.path.join(ROOT, "profiles", "gumbel.log")
be = M0Backend.from_state_dict(bench.R24_320, random_state_dict(bench.R24_320, seed=0, varied=True))


def run_plies(e, games, n_plies, sims):
    target = e.stats()["plies"] + n_plies * games
    passes = 0
    while e.stats()["plies"] < target and passes < 8 * n_plies * (sims + 2):
        e.step(1)
        passes += 1


for games in (256, 1024):
    for sims in (16, 32, 64):
        for root in ("puct", "gumbel"):
            cfg = json.loads(json.dumps(bench.SELFPLAY_CFG))
            cfg["selfplay"]["num_simulations"] = sims
            if root == "gumbel":
                cfg["mcts"]["gumbel"] = {"enabled": True, "max_considered": 16}
            e = eng.SelfplayEngine(be, eng.selfplay_cfg_from_dict(cfg, concurrent_games=games, total_games=0, leaves_per_step=sims,
                                                                  virtual_loss_active=True, record_games=False, eval_cache=False))
            g = eng.gumbel_cfg_from_dict(cfg)
            if g is not None:
                e.set_gumbel(g)
            run_plies(e, games, warmup, sims)
            torch.cuda.synchronize()
            s0, t0 = e.stats(), time.perf_counter()
            run_plies(e, games, plies, sims)
            torch.cuda.synchronize()
            dt, s1 = time.perf_counter() - t0, e.stats()
            e.close()
            d = {k: s1[k] - s0[k] for k in ("plies", "evals", "steps", "sims")}
            line = json.dumps({"root": root, "sims": sims, "games": games, "max_considered": 16 if root == "gumbel" else None,
                               "plies_timed_per_game": plies, "seconds": round(dt, 3),
                               "searched_plies_per_s": round(d["plies"] / dt, 1), "evals_per_s": round(d["evals"] / dt),
                               "rows_per_forward": round(d["evals"] / max(1, d["steps"]), 1),
                               "passes_per_search": round(d["steps"] * games / max(1, d["plies"]), 2),
                               "sims_per_ply": round(d["sims"] / max(1, d["plies"]), 1)})
            print(line, flush=True)
            with open(LOG, "a") as f:
                f.write(line + "\n")
be.close()
