#!/usr/bin/env python3
"""Measurements of the SSL score (matrix0_amd/score.py with ssl=...), appended to profiles/ssl_score.log:

  a  ssl_score_kernel alone on resident inputs (m0_ssl_score_bench), all five tasks, at 4096 and 24576 rows, targets taken from
     the planes and stored: microseconds per launch, GB/s over the bytes a launch must move, and that as a share of the
     achievable HBM bandwidth (6.3 TB/s: a float4 copy on an MI355X)
  b  on a random R24-320 network with the five heads: milliseconds per forward with and without the heads
     (m0_net_bench_forward, resident input), and rows/s of score_shards over a temporary store without ssl and with
     ssl="planes", in one process

Each step runs as a child process under its own time limit, and a step that fails ends the run.
`python tools/bench_ssl_score.py [--batch 4096] [--log profiles/ssl_score.log] [--commit TEXT] [--note TEXT] [--limit SECONDS]`"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
HBM_ACHIEVABLE_GBS = 6300.0
TASKS = ["piece", "threat", "pin", "fork", "control"]
CFG = dict(planes=19, channels=320, blocks=24, attention_heads=20, policy_size=4672, norm="group", activation="silu", preact=True,
           policy_factor_rank=128, self_supervised=True, ssl_tasks=TASKS)
OPTS = dict(label_smoothing=0.05, value_loss="huber", huber_delta=1.0)


def step_a(_):
    import ctypes as C
    from matrix0_amd import _lib
    out = []
    for B in (4096, 24576):
        for from_planes in (1, 0):
            us, nbytes = C.c_float(0), C.c_double(0)
            _lib.check(_lib.lib().m0_ssl_score_bench(0, B, 31, from_planes, 50, C.byref(us), C.byref(nbytes)), "m0_ssl_score_bench")
            gbs = nbytes.value / us.value / 1e3
            out.append({"B": B, "targets": "planes" if from_planes else "stored", "launches": 50, "us_per_launch": round(us.value, 1),
                        "MB_per_launch": round(nbytes.value / 1e6, 1), "GB_per_s": round(gbs, 1),
                        "share_of_achievable_hbm": round(gbs / HBM_ACHIEVABLE_GBS, 3)})
    return {"achievable_GB_per_s": HBM_ACHIEVABLE_GBS, "runs": out}


def step_b(B):
    import numpy as np
    from bench_score import rows
    from matrix0_amd import score as sc
    from matrix0_amd.backend import M0Backend
    from matrix0_amd.data_writer import ShardIndex
    from matrix0_amd.weights import random_state_dict
    be = M0Backend.from_state_dict(CFG, random_state_dict(CFG, seed=0, varied=True))
    ms = {}
    for with_ssl in (False, True, False, True):                                    # alternating; the later pair is kept
        ms[with_ssl] = be.bench_forward(B, 5, with_ssl)
    x, pi, z, mask = rows(2 * B)
    x[:, :12] = 0
    sq = np.random.default_rng(2).integers(0, 12, size=(2 * B, 64))
    occupied = np.random.default_rng(3).random((2 * B, 64)) < 0.4
    np.put_along_axis(x.reshape(2 * B, 19, 64)[:, :12], sq[:, None], occupied[:, None].astype(np.float32), axis=1)   # one piece per square
    with tempfile.TemporaryDirectory() as d:
        index = ShardIndex(d)
        for k in range(2):
            path = os.path.join(d, f"shard_{k}.npz")
            np.savez(path, s=x[k * B:(k + 1) * B], pi=pi[k * B:(k + 1) * B], z=z[k * B:(k + 1) * B], legal_mask=mask[k * B:(k + 1) * B])
            index.add(path, B, "selfplay")
        rate = {}
        sc.score_shards(d, be, batch=B, ssl="planes", **OPTS)                       # workspace, staging, page cache
        for ssl in (None, "planes", None, "planes"):
            t0 = time.perf_counter()
            r = sc.score_shards(d, be, batch=B, ssl=ssl, **OPTS)
            rate[ssl] = 2 * B / (time.perf_counter() - t0)
    be.close()
    x = r["ssl"]
    return {"B": B, "forward_ms": round(ms[False], 2), "forward_with_ssl_heads_ms": round(ms[True], 2),
            "heads_share_of_forward": round(ms[True] / ms[False] - 1, 4), "score_shards_rows": 2 * B,
            "score_shards_rows_per_s": round(rate[None]), "score_shards_ssl_planes_rows_per_s": round(rate["planes"]),
            "ssl_scored": x["scored"], "ssl_flags": x["flags"], "mean_piece_loss": round(x["loss"]["piece"], 4)}


STEPS = {"a": ("ssl_score_kernel alone, five tasks", step_a), "b": ("forward with the heads; score_shards with ssl='planes'", step_b)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096, help="rows per forward of step b; its store holds twice as many")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "ssl_score.log"))
    ap.add_argument("--commit", default=None, help="what the header says was measured (default: git rev-parse --short HEAD)")
    ap.add_argument("--note", default="", help="appended to the header: bench.py's value on this commit and on its parent")
    ap.add_argument("--limit", type=int, default=300, help="seconds per step")
    ap.add_argument("--step", choices=list(STEPS), default=None, help="run one step in this process and print its JSON line")
    args = ap.parse_args()
    if args.step:
        print(json.dumps(STEPS[args.step][1](args.batch)), flush=True)
        return 0
    commit = args.commit
    if commit is None:
        got = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True)
        commit = got.stdout.strip() if got.returncode == 0 else "unknown"
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "a") as log:
        log.write(f"# tools/bench_ssl_score.py --batch {args.batch}; commit {commit}; {time.strftime('%Y-%m-%d %H:%M:%S')}; "
                  f"options {json.dumps(OPTS)}; R24-320 with five SSL heads, random weights" + (f"; {args.note}" if args.note else "") + "\n")
        log.flush()
        for key, (what, _) in STEPS.items():
            try:
                got = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", key, "--batch", str(args.batch)],
                                     capture_output=True, text=True, timeout=args.limit)
            except subprocess.TimeoutExpired:
                log.write(f"{key} ({what}): no result within {args.limit} s; the run ends here\n")
                return 1
            if got.returncode != 0:
                log.write(f"{key} ({what}): exit status {got.returncode}; the run ends here\n")
                sys.stderr.write(got.stderr[-2000:])
                return 1
            line = got.stdout.strip().splitlines()[-1]
            log.write(f"{key} ({what}): {line}\n")
            log.flush()
            print(key, line, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
