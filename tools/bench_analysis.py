"""Throughput of the analysis engine on one MI355X (matrix0_amd/analysis.py), random R24-320 weights, 256 tree slots, the
labelled positions of tests/golden/stockfish_best_moves.json.gz cycled to --positions submissions.

  search    Analyzer.analyse, --sims simulations, --leaves leaves per tree and step: positions/s and evaluations/s.
            Yardstick: the evaluations/s `python bench.py` prints on the same build and box (same kernels, same pass
            shape); the analysis figure differs by its refill and harvest work.  Pass it with --selfplay-evals-per-s to
            have the ratio in the line.
  baseline  the same positions through the split-step search API, the only FEN-addressed path before the analysis engine:
            m0_search_begin / _select (leaf planes to the host as f32) / infer_np / _expand (logits from the host), 256 slots
            at a time.  --baseline-positions limits it (it is slow by construction).
  policy    Analyzer.evaluate: positions/s, against m0_net_bench_forward at the same batch size (the gap is the encode,
            the policy kernel and the copies).

Every mode runs --repeats times, alternating, after one untimed warm-up; one JSON line per run goes to stdout and to --log."""
from __future__ import annotations

import argparse
import gzip
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from bench import R24_320, SELFPLAY_CFG  # noqa: E402


def positions(n):
    rows = json.load(gzip.open(os.path.join(ROOT, "tests", "golden", "stockfish_best_moves.json.gz"), "rt"))
    return [rows[i % len(rows)][0] for i in range(n)]


def run_search(be, cfg, fens, sims, slots):
    from matrix0_amd import analysis
    an = analysis.Analyzer(be, cfg, slots=slots, max_sims=sims)
    t0 = time.perf_counter()
    res = an.analyse(fens, sims)
    dt = time.perf_counter() - t0
    st = an.stats()
    an.close()
    searched = sum(1 for r in res if r["status"] == "ok")
    return {"mode": "search", "positions": len(fens), "searched": searched, "sims": sims, "secs": dt,
            "positions_per_s": len(fens) / dt, "evals_per_s": st["evals"] / dt, "evals": int(st["evals"]),
            "overflows": int(st["arena_overflows"])}


def run_baseline(be, cfg, fens, sims, slots):
    from matrix0_amd import engine as eng
    c = eng.selfplay_cfg_from_dict(cfg, concurrent_games=slots, record_games=False)
    c.num_simulations = sims
    e = eng.SelfplayEngine(None, c)
    evals = 0
    t0 = time.perf_counter()
    for base in range(0, len(fens), slots):
        chunk = fens[base: base + slots]
        live = []
        for g, fen in enumerate(chunk):
            try:
                e.search_begin(g, fen, sims, False, base + g)
                live.append(g)
            except Exception:
                pass
        while True:
            planes = e.search_select()
            if planes.shape[0]:
                lg, v = be.infer_np(planes)
            else:                                     # a pass of terminal leaves only, or every search has finished
                if all(e.search_result(g)["finished"] for g in live):
                    break
                lg, v = np.zeros((0, 4672), np.float32), np.zeros((0,), np.float32)
            evals += planes.shape[0]
            e.search_expand(lg, v)
        for g in live:
            e.search_result(g)
    dt = time.perf_counter() - t0
    e.close()
    return {"mode": "baseline", "positions": len(fens), "sims": sims, "secs": dt, "positions_per_s": len(fens) / dt,
            "evals_per_s": evals / dt, "evals": evals}


def run_policy(be, cfg, fens, slots, leaves):
    import ctypes as C
    from matrix0_amd import _lib, analysis
    an = analysis.Analyzer(be, cfg, slots=slots, multipv=5, pv_len=1)
    t0 = time.perf_counter()
    an.evaluate(fens, topk=5)
    dt = time.perf_counter() - t0
    an.close()
    batch = slots * (leaves + 1)
    ms = C.c_float(0)
    _lib.check(_lib.lib().m0_net_bench_forward(be.handle, batch, 5, 0, C.byref(ms)), "m0_net_bench_forward")
    fwd = batch / (ms.value / 1e3)
    return {"mode": "policy", "positions": len(fens), "secs": dt, "positions_per_s": len(fens) / dt, "batch": batch,
            "forward_positions_per_s": fwd, "ratio_to_forward": (len(fens) / dt) / fwd}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--positions", type=int, default=2048)
    ap.add_argument("--baseline-positions", type=int, default=256)
    ap.add_argument("--policy-positions", type=int, default=49152)
    ap.add_argument("--sims", type=int, default=800)
    ap.add_argument("--leaves", type=int, default=96)
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--modes", default="search,baseline,policy")
    ap.add_argument("--selfplay-evals-per-s", type=float, default=0.0, help="evaluations/s of bench.py on this build and box")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "analysis.log"))
    args = ap.parse_args()
    from matrix0_amd.backend import M0Backend
    from matrix0_amd.weights import random_state_dict
    be = M0Backend.from_state_dict(R24_320, random_state_dict(R24_320, seed=0, varied=True))
    cfg = json.loads(json.dumps(SELFPLAY_CFG))
    cfg["mcts"]["inference_batch_size"] = args.leaves
    cfg["mcts"]["playout_random_frac"] = 0.0
    modes = [m for m in args.modes.split(",") if m]
    runs = {"search": lambda n: run_search(be, cfg, positions(n or args.positions), args.sims, args.slots),
            "baseline": lambda n: run_baseline(be, cfg, positions(n or args.baseline_positions), args.sims, args.slots),
            "policy": lambda n: run_policy(be, cfg, positions(n or args.policy_positions), args.slots, args.leaves)}
    for m in modes:                                   # warm-up: workspaces, code objects, clocks
        runs[m](args.slots)
    with open(args.log, "a") as log:
        for rep in range(args.repeats):
            for m in modes:                           # alternating, so that drift hits every mode alike
                out = runs[m](0)
                out["repeat"] = rep
                if m == "search" and args.selfplay_evals_per_s > 0:
                    out["selfplay_evals_per_s"] = args.selfplay_evals_per_s
                    out["ratio_to_selfplay"] = out["evals_per_s"] / args.selfplay_evals_per_s
                line = json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in out.items()})
                print(line, flush=True)
                log.write(line + "\n")
    be.close()


if __name__ == "__main__":
    main()
