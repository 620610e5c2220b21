"""Throughput of reanalyse on one MI355X (matrix0_amd/reanalyse.py), random R24-320 weights, the labelled positions of
tests/golden/stockfish_best_moves.json.gz cycled to --positions rows (their planes and legal masks, as a shard holds them).

  planes    reanalyse_arrays: rows submitted as planes (decoded on the device), --sims simulations, every root child's visits
            brought back, pi / z rebuilt: positions/s and evaluations/s.
  fens      the yardstick, on the same build and box: Analyzer.analyse of the same positions as FENs at the same --sims and
            --slots (tools/bench_analysis.py search mode).  Only the submission and the visit harvest differ, so the two are
            expected inside the 1-6 % box-to-box spread of DESIGN.md section 6.
  decode    the decode kernel alone against its neighbour: encoding.decode_planes and encoding.encode_fens over the same rows,
            rows/s, both through their C calls (host copies included: planes and masks go up for one, come down for the other).

Every mode runs --repeats times, alternating, after one untimed warm-up; one JSON line per run goes to stdout and to --log."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from bench import R24_320, SELFPLAY_CFG  # noqa: E402
from tools.bench_analysis import positions  # noqa: E402


def rows_of(fens):
    """(s, pi, z, legal_mask) as an imported shard holds these positions: one-hot pi on the first legal move, z = 0."""
    from matrix0_amd import encoding
    s, mask, _ = encoding.encode_fens(fens, want_moves=False)
    mask = mask.astype(np.uint8)
    pi = np.zeros((len(fens), 4672), np.float32)
    pi[np.arange(len(fens)), mask.argmax(axis=1)] = 1.0
    return s, pi, np.zeros(len(fens), np.float32), mask


def run_planes(be, cfg, rows, sims, slots):
    from matrix0_amd import analysis, reanalyse
    an = analysis.Analyzer(be, cfg, slots=slots, max_sims=sims)
    t0 = time.perf_counter()
    _, _, rep = reanalyse.reanalyse_arrays(*rows, sims=sims, analyzer=an)
    dt = time.perf_counter() - t0
    st = an.stats()
    an.close()
    n = len(rows[0])
    return {"mode": "planes", "positions": n, "searched": rep["searched"], "kept": rep["kept"], "sims": sims, "secs": dt,
            "positions_per_s": n / dt, "evals_per_s": st["evals"] / dt, "evals": int(st["evals"]),
            "overflows": int(st["arena_overflows"])}


def run_fens(be, cfg, fens, sims, slots):
    from tools.bench_analysis import run_search
    out = run_search(be, cfg, fens, sims, slots)
    out["mode"] = "fens"
    return out


def run_decode(rows, fens):
    from matrix0_amd import encoding
    t0 = time.perf_counter()
    d = encoding.decode_planes(rows[0], rows[3])
    t1 = time.perf_counter()
    encoding.encode_fens(fens, want_moves=False)
    t2 = time.perf_counter()
    n = len(fens)
    return {"mode": "decode", "rows": n, "bad_status": int(np.count_nonzero(d["status"])), "decode_rows_per_s": n / (t1 - t0),
            "encode_rows_per_s": n / (t2 - t1), "decode_secs": t1 - t0, "encode_secs": t2 - t1}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--positions", type=int, default=2048)
    ap.add_argument("--decode-rows", type=int, default=65536)
    ap.add_argument("--sims", type=int, default=800)
    ap.add_argument("--leaves", type=int, default=96)
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--modes", default="planes,fens,decode")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "reanalyse.log"))
    args = ap.parse_args()
    from matrix0_amd.backend import M0Backend
    from matrix0_amd.weights import random_state_dict
    be = M0Backend.from_state_dict(R24_320, random_state_dict(R24_320, seed=0, varied=True))
    cfg = json.loads(json.dumps(SELFPLAY_CFG))
    cfg["mcts"]["inference_batch_size"] = args.leaves
    cfg["mcts"]["playout_random_frac"] = 0.0
    modes = [m for m in args.modes.split(",") if m]
    fens, small = positions(args.positions), positions(args.slots)
    rows, small_rows = rows_of(fens), rows_of(small)
    dfens = positions(args.decode_rows) if "decode" in modes else []
    drows = rows_of(dfens) if dfens else None
    runs = {"planes": lambda warm: run_planes(be, cfg, small_rows if warm else rows, args.sims, args.slots),
            "fens": lambda warm: run_fens(be, cfg, small if warm else fens, args.sims, args.slots),
            "decode": lambda warm: run_decode(drows, dfens)}
    for m in modes:                                   # warm-up: workspaces, code objects, clocks
        runs[m](True)
    with open(args.log, "a") as log:
        for rep in range(args.repeats):
            for m in modes:                           # alternating, so that drift hits every mode alike
                out = runs[m](False)
                out["repeat"] = rep
                line = json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in out.items()})
                print(line, flush=True)
                log.write(line + "\n")
    be.close()


if __name__ == "__main__":
    main()
