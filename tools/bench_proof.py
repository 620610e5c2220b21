#!/usr/bin/env python3
"""The proof search (include/m0_proof.h) beside the search without it, through the split-step calls with the hash evaluator of
tests/hash_net.py (a pure function of the position: both modes see the same values, and its time is not counted).

Two measurements, each against the mode off in the same run, one JSON line per position written to profiles/proof.log (a run replaces the file):
  proven   simulations, passes and milliseconds inside the engine's calls until the root is proven, on the six solved positions
           of tests/proof_ref.py and a dozen 3-man endings with the tables attached; mode off: the whole budget.
  quiet    milliseconds inside the engine's calls per 800-simulation search of the middlegames of tests/test_search_gpu.py,
           where nothing is proven: what the extra scan of the children's proofs costs.

usage: bench_proof.py [sims=800] [leaves=16] [repeats=5]"""
import json, os, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np
from matrix0_amd import engine as eng
from matrix0_amd.tablebase import Tablebase
from tests import proof_ref as pr
from tests.hash_net import HashNet
from tests.test_search_gpu import FENS, MCTS

sims = int(sys.argv[1]) if len(sys.argv) > 1 else 800
leaves = int(sys.argv[2]) if len(sys.argv) > 2 else 16
repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 5
LOG = os.path.join(ROOT, "profiles", "proof.log")
ENDINGS = ["8/8/8/4k3/8/8/8/KQ6 w - - 0 1", "7k/8/8/8/8/8/8/KQ6 w - - 0 1", "8/8/3k4/8/8/8/1Q6/K7 w - - 0 1",
           "4k3/8/8/8/8/8/8/Q3K3 w - - 0 1", "8/8/8/4k3/8/8/4K3/R7 w - - 0 1", "7k/8/8/8/8/8/8/KR6 w - - 0 1",
           "8/8/3k4/8/8/8/1R6/K7 w - - 0 1", "4k3/8/8/8/8/8/8/R3K3 w - - 0 1", "8/8/8/4k3/8/8/8/KQ6 b - - 0 1",
           "7k/8/8/8/8/8/8/KQ6 b - - 0 1", "8/8/8/4k3/8/8/4K3/R7 b - - 0 1", "7k/8/8/8/8/8/8/KR6 b - - 0 1"]
Z0 = (np.zeros((0, 4672), np.float32), np.zeros((0,), np.float32))


def search(fen, proof, tb, uid):
    """One search to its end: (simulations, passes, milliseconds in the engine, root state)"""
    cfg = eng.selfplay_cfg_from_dict({"seed": 1234, "mcts": dict(MCTS, inference_batch_size=leaves),
                                      "selfplay": {"num_simulations": sims}}, concurrent_games=1, virtual_loss_active=True)
    e = eng.SelfplayEngine(None, cfg)
    if proof:
        e.set_proof()
    if tb is not None:
        e.set_search_tablebase(tb, 3)
    net = HashNet(seed=41, sharp=2.0, vscale=0.3)
    e.search_begin(0, fen, sims, False, uid)
    ms, passes = 0.0, 0
    for _ in range(sims + 8):
        t0 = time.perf_counter()
        planes = e.search_select()
        ms += (time.perf_counter() - t0) * 1e3
        lg, v = net.infer_np(planes) if planes.shape[0] else Z0
        t0 = time.perf_counter()
        e.search_expand(lg, v)
        fin = e.search_result(0)["finished"]
        ms += (time.perf_counter() - t0) * 1e3
        passes += 1
        if fin:
            break
    res = e.search_result(0)
    state = e.search_proof_result(0)["state"] if proof else "off"
    e.close()
    return int(res["n"].sum()), passes, ms, state


def measure(kind, fen, tb):
    row = {"bench": "proof", "kind": kind, "fen": fen, "sims": sims, "leaves": leaves, "repeats": repeats}
    for mode, proof in (("on", True), ("off", False)):
        runs = [search(fen, proof, tb, 7000 + r) for r in range(repeats)]
        row[mode] = {"sims": [r[0] for r in runs], "passes": [r[1] for r in runs], "ms": [round(r[2], 3) for r in runs],
                     "state": sorted(set(r[3] for r in runs))}
    print(json.dumps(row), flush=True)
    with open(LOG, "a") as f:
        f.write(json.dumps(row) + "\n")


open(LOG, "w").close()                               # a run replaces the log
search(FENS[0], True, None, 1)                       # first-launch costs stay out of the numbers
tb3 = Tablebase.build(3, 0)
for fen, _, _, _ in pr.POSITIONS:
    measure("proven", fen, None)
for fen in ENDINGS:
    measure("proven-tables", fen, tb3)
for fen in FENS[:4]:
    measure("quiet", fen, None)
tb3.close()
