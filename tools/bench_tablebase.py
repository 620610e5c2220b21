#!/usr/bin/env python3
"""Build time of the generated endgame tablebases on one GPU: the 3-man set, then the full 4-man set, with the number of
sweeps, the largest d and the milliseconds of every table.  Writes profiles/tablebase.log.

    python tools/bench_tablebase.py [--device 0] [--max-men 4] [--out profiles/tablebase.log]

--search measures the tables inside the search instead: a self-play engine on the benchmark network plays from a book of 5-man
positions, once with the 4-man set attached to the search (m0_selfplay_set_search_tablebase) and once with nothing attached;
upload time, plies/s, evaluations/s and table leaves per ply are appended to profiles/tb_search.log.

    python tools/bench_tablebase.py --search [--games 256] [--steps 200] [--sims 200] [--cache tb4.m0tb]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


# 5-man positions one capture or promotion away from the 4-man tables (no castling rights)
BOOK5 = ["8/8/4k3/3r4/8/2B5/1Q6/4K3 w - - 0 1", "8/5k2/8/2n5/8/3R4/1P6/4K3 w - - 0 1", "4k3/1p6/8/8/2R5/8/5P2/4K3 b - - 0 1",
         "8/2k5/8/3q4/8/2N5/3Q4/3K4 w - - 0 1", "8/8/3k4/8/2b1r3/8/3R4/2K5 b - - 0 1", "8/6k1/5p2/8/3N4/8/1P6/1K6 w - - 0 1",
         "3k4/8/8/2p5/8/1R6/8/1K2B3 w - - 0 1", "8/8/2k5/8/1n1N4/8/P7/K7 b - - 0 1"]


def search_mode(a) -> int:
    import bench
    from matrix0_amd import engine as eng
    from matrix0_amd.backend import M0Backend
    from matrix0_amd.tablebase import Tablebase
    from matrix0_amd.weights import random_state_dict
    tb = Tablebase.cached(a.cache, a.max_men, a.device)
    cfg_dict = {"seed": 7, "mcts": {"legal_softmax": True, "inference_batch_size": 96},
                "selfplay": {"num_simulations": a.sims, "max_game_len": 60, "opening_random_plies": 0}}
    lines = [f"search mode: {a.games} games, {a.steps} steps, {a.sims} simulations, book of {len(BOOK5)} 5-man positions, "
             f"tables up to {tb.max_men} men"]
    for attached in (True, False):
        be = M0Backend.from_state_dict(bench.R24_320, random_state_dict(bench.R24_320, seed=0, varied=True), device_index=a.device)
        e = eng.SelfplayEngine(be, eng.selfplay_cfg_from_dict(cfg_dict, concurrent_games=a.games, record_games=False))
        e.set_openings(BOOK5)
        upload = 0.0
        if attached:
            t0 = time.perf_counter()
            e.set_search_tablebase(tb, a.max_men)
            upload = time.perf_counter() - t0
        e.step(a.warmup)
        s0, t0 = e.stats(), time.perf_counter()
        leaves0 = e.tb_leaves()
        e.step(a.steps)
        s1, secs = e.stats(), time.perf_counter() - t0
        plies, evals, leaves = s1["plies"] - s0["plies"], s1["evals"] - s0["evals"], e.tb_leaves() - leaves0
        lines.append(f"  tables {'attached' if attached else 'detached'}: upload {upload:.3f} s, {plies / secs:.1f} plies/s, "
                     f"{evals / secs:.0f} evaluations/s, {leaves / max(1, plies):.1f} table leaves per ply, "
                     f"{e.tb_adjudications()} games adjudicated, {secs:.2f} s")
        e.close()
        be.close()
    tb.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.search_out), exist_ok=True)
    with open(a.search_out, "a") as f:
        f.write(text)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--max-men", type=int, default=4, choices=(3, 4))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tablebase.log"))
    ap.add_argument("--search", action="store_true", help="measure the tables inside the search (appends to --search-out)")
    ap.add_argument("--search-out", default=os.path.join(ROOT, "profiles", "tb_search.log"))
    ap.add_argument("--cache", default=None, help="--search: cache file of the tables (built and saved there when absent)")
    ap.add_argument("--games", type=int, default=256)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--sims", type=int, default=200)
    a = ap.parse_args()
    if a.search:
        return search_mode(a)
    from matrix0_amd.tablebase import Tablebase
    lines = []
    for men in range(3, a.max_men + 1):
        t0 = time.perf_counter()
        tb = Tablebase.build(men, a.device)
        secs = time.perf_counter() - t0
        info = tb.info()
        lines.append(f"build max_men={men}: {len(info)} tables, {sum(2 * 64 ** len(i['sig']) for i in info) / 2 ** 20:.0f} MiB, "
                     f"{secs:.3f} s wall (kernels, sweep counters and the copy of every table to the host)")
        for i in info:
            lines.append(f"  {i['sig']:<5} sweeps {i['sweeps']:>3}  largest d {i['max_d']:>3}  {i['build_ms']:9.1f} ms")
        tb.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
