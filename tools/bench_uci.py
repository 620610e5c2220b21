"""What one tree costs on one MI355X: the UCI engine's search shape (matrix0_amd/uci.py) -- ONE tree slot, --leaves leaves per
pass (default 96), random R24-320 weights.  No threshold is attached to any figure here: they are recorded because nobody had
measured a one-tree pass on this network.

  single    a single-position search of --sims simulations with keep: nodes/s and ms per pass (select -> network -> expand
            of one tree, at most leaves + 1 batch rows), with a peek every --peek-every passes as the front end's `info`
            lines take it.
  reuse     a fixed 20-ply line played out: every position is searched with --sims simulations, the next position is the
            last one plus the line's next move, continued in the held tree (continue_search).  Per ply the visits carried
            over, and their share of the visits of the search they came from.

Every mode runs --repeats times after one untimed warm-up; one JSON line per run goes to stdout and to --log."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import R24_320, SELFPLAY_CFG  # noqa: E402

START_FEN = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1"
# a Ruy Lopez main line, 20 plies
LINE = ("e2e4 e7e5 g1f3 b8c6 f1b5 a7a6 b5a4 g8f6 e1g1 f8e7 f1e1 b7b5 a4b3 d7d6 c2c3 e8g8 h2h3 c6a5 b3c2 c7c5").split()


def make_engine(be, cfg, leaves, sims):
    from matrix0_amd import uci
    opts = dict({k: v[1] for k, v in uci.OPTIONS.items()}, Leaves=leaves, MaxNodes=sims)
    return uci.make_engine(be, cfg, opts)[0]


def run_to_answer(e, on_pass=None):
    passes = 0
    while e.pending():
        e.step(1)
        passes += 1
        if on_pass:
            on_pass(passes)
    return e.poll(), passes


def run_single(be, cfg, leaves, sims, peek_every):
    e = make_engine(be, cfg, leaves, sims)
    peeks = [0]

    def on_pass(k):
        if peek_every > 0 and k % peek_every == 0 and e.pending():
            e.peek(1)
            peeks[0] += 1

    e.submit(START_FEN, LINE[:8], sims=sims, id=1, keep=True)
    t0 = time.perf_counter()
    r, passes = run_to_answer(e, on_pass)
    dt = time.perf_counter() - t0
    e.close()
    return {"mode": "single", "leaves": leaves, "sims": sims, "passes": passes, "peeks": peeks[0], "secs": dt,
            "nodes_per_s": r["sims"] / dt, "ms_per_pass": 1e3 * dt / passes, "evals": r["evals"], "root_n": r["root_n"],
            "overflow": r["overflow"]}


def run_reuse(be, cfg, leaves, sims):
    e = make_engine(be, cfg, leaves, sims)
    plies = []
    t0 = time.perf_counter()
    e.submit(START_FEN, [], sims=sims, id=1, keep=True)
    r, _ = run_to_answer(e)
    for k, mv in enumerate(LINE):
        reused = e.continue_search(k + 1, [mv], sims=sims, id=k + 2, keep=True)
        plies.append({"ply": k + 1, "move": mv, "reused_n": reused, "share": reused / max(1, r["root_n"])})
        r, _ = run_to_answer(e)
    dt = time.perf_counter() - t0
    e.close()
    shares = [p["share"] for p in plies]
    return {"mode": "reuse", "leaves": leaves, "sims": sims, "plies": len(plies), "secs": dt,
            "mean_share_carried_over": sum(shares) / len(shares), "min_share": min(shares), "max_share": max(shares),
            "reused_n": [p["reused_n"] for p in plies], "overflow": r["overflow"]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sims", type=int, default=800)
    ap.add_argument("--leaves", type=int, default=96)
    ap.add_argument("--peek-every", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--modes", default="single,reuse")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "uci.log"))
    args = ap.parse_args()
    from matrix0_amd.backend import M0Backend
    from matrix0_amd.weights import random_state_dict
    be = M0Backend.from_state_dict(R24_320, random_state_dict(R24_320, seed=0, varied=True))
    cfg = json.loads(json.dumps(SELFPLAY_CFG))
    cfg["mcts"]["playout_random_frac"] = 0.0
    runs = {"single": lambda: run_single(be, cfg, args.leaves, args.sims, args.peek_every),
            "reuse": lambda: run_reuse(be, cfg, args.leaves, args.sims)}
    modes = [m for m in args.modes.split(",") if m]
    for m in modes:                                   # warm-up: workspaces, code objects, clocks
        runs[m]()
    with open(args.log, "a") as log:
        for rep in range(args.repeats):
            for m in modes:
                out = dict(runs[m](), repeat=rep)
                line = json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in out.items()})
                print(line, flush=True)
                log.write(line + "\n")
    be.close()


if __name__ == "__main__":
    main()
