#!/usr/bin/env python3
"""Three measurements of the training-loss score (matrix0_amd/score.py), appended to profiles/score.log:

  a  score_rows_kernel alone at B rows on resident inputs (m0_score_bench): microseconds per launch, GB/s over the bytes a launch
     must move, and that as a share of the achievable HBM bandwidth (6.3 TB/s: a float4 copy on an MI355X)
  b  M0Backend.score (m0_net_score: host rows in, forward, loss on the device, 8 floats per row out) in positions/s, beside
     m0_net_bench_forward (the forward alone, resident input) at the same B
  c  the same rows through infer_np and a numpy float32 loss on the host: what the package could do before m0_net_score

Each step runs as a child process under its own time limit, and a step that fails ends the run.
`python tools/bench_score.py [--batch 24576] [--log profiles/score.log] [--commit TEXT] [--limit SECONDS]`"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
HBM_ACHIEVABLE_GBS = 6300.0
CFG = dict(planes=19, channels=320, blocks=24, attention_heads=20, policy_size=4672, norm="group", activation="silu", preact=True,
           policy_factor_rank=128, self_supervised=False)
OPTS = dict(label_smoothing=0.05, value_loss="huber", huber_delta=1.0)


def rows(B):
    """seeded planes, soft pi on 8 of about 35 legal moves, z, legal masks"""
    import numpy as np
    rng = np.random.default_rng(1)
    x = np.zeros((B, 19, 8, 8), np.float32)
    x[:, :12] = (rng.random((B, 12, 8, 8)) < 0.08).astype(np.float32)
    x[:, 12:17] = (rng.random((B, 5, 1, 1)) < 0.5).astype(np.float32)
    x[:, 17:] = rng.random((B, 2, 1, 1)).astype(np.float32)
    cols = rng.integers(0, 4672, size=(B, 35))
    mask = np.zeros((B, 4672), np.uint8)
    np.put_along_axis(mask, cols, 1, axis=1)
    pi = np.zeros((B, 4672), np.float32)
    np.put_along_axis(pi, cols[:, :8], rng.random((B, 8)).astype(np.float32) + 0.01, axis=1)
    pi /= pi.sum(axis=1, keepdims=True)
    return x, pi, rng.integers(-1, 2, size=B).astype(np.float32), mask


def host_loss(logits, value, pi, z, mask, label_smoothing, huber_delta):
    """train.py:436-549 per row in numpy float32 (legal mask | pi > 0, smoothing over the support, smooth_l1)"""
    import numpy as np
    sup = (mask != 0) | (pi > 0)
    lg = np.where(sup, logits, np.float32(-1e9))
    lg -= lg.max(axis=1, keepdims=True)
    logp = lg - np.log(np.exp(lg).sum(axis=1, keepdims=True))
    pi_s = (1 - label_smoothing) * pi + label_smoothing * sup / np.maximum(sup.sum(axis=1, keepdims=True), 1)
    policy = -(pi_s * np.where(sup, logp, 0)).sum(axis=1)
    d = np.abs(value - z)
    return policy, np.where(d < huber_delta, 0.5 * d * d / huber_delta, d - 0.5 * huber_delta)


def backend():
    from matrix0_amd.backend import M0Backend
    from matrix0_amd.weights import random_state_dict
    return M0Backend.from_state_dict(CFG, random_state_dict(CFG, seed=0, varied=True))


def step_a(B):
    import ctypes as C
    from matrix0_amd import _lib
    us, nbytes = C.c_float(0), C.c_double(0)
    _lib.check(_lib.lib().m0_score_bench(0, B, 20, C.byref(us), C.byref(nbytes)), "m0_score_bench")
    gbs = nbytes.value / us.value / 1e3
    return {"B": B, "launches": 20, "us_per_launch": round(us.value, 1), "MB_per_launch": round(nbytes.value / 1e6, 1),
            "GB_per_s": round(gbs, 1), "share_of_achievable_hbm": round(gbs / HBM_ACHIEVABLE_GBS, 3), "achievable_GB_per_s": HBM_ACHIEVABLE_GBS}


def step_b(B):
    be = backend()
    x, pi, z, mask = rows(B)
    be.score(x, pi, z, mask, **OPTS)                        # workspace, staging
    n = 3
    t0 = time.perf_counter()
    for _ in range(n):
        r = be.score(x, pi, z, mask, **OPTS)
    dt = (time.perf_counter() - t0) / n
    ms_fwd = be.bench_forward(B, 3)
    return {"B": B, "calls": n, "score_ms_per_call": round(dt * 1e3, 2), "score_positions_per_s": round(B / dt),
            "forward_ms_device_resident": round(ms_fwd, 2), "forward_positions_per_s": round(B / ms_fwd * 1e3),
            "host_MB_in_per_call": round((x.nbytes + pi.nbytes + z.nbytes + mask.nbytes) / 1e6, 1),
            "host_MB_out_per_call": round(r.nbytes / 1e6, 2), "mean_policy_loss": round(float(r[:, 0].mean()), 4)}


def step_c(B):
    be = backend()
    x, pi, z, mask = rows(B)
    be.infer_np(x)
    n, t_infer, t_loss = 2, 0.0, 0.0
    for _ in range(n):
        t0 = time.perf_counter()
        p, v = be.infer_np(x)
        t1 = time.perf_counter()
        policy, _ = host_loss(p, v, pi, z, mask, OPTS["label_smoothing"], OPTS["huber_delta"])
        t_loss += time.perf_counter() - t1
        t_infer += t1 - t0
    dt = (t_infer + t_loss) / n
    return {"B": B, "calls": n, "infer_np_ms_per_call": round(t_infer / n * 1e3, 2), "numpy_loss_ms_per_call": round(t_loss / n * 1e3, 2),
            "positions_per_s": round(B / dt), "host_MB_out_per_call": round((p.nbytes + v.nbytes) / 1e6, 1),
            "mean_policy_loss": round(float(policy.mean()), 4)}


STEPS = {"a": ("score_rows_kernel alone", step_a), "b": ("m0_net_score beside m0_net_bench_forward", step_b),
         "c": ("infer_np + numpy float32 loss on the host", step_c)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=24576)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "score.log"))
    ap.add_argument("--commit", default=None, help="what the header says was measured (default: git rev-parse --short HEAD)")
    ap.add_argument("--limit", type=int, default=420, help="seconds per step")
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
        log.write(f"# tools/bench_score.py --batch {args.batch}; commit {commit}; {time.strftime('%Y-%m-%d %H:%M:%S')}; "
                  f"options {json.dumps(OPTS)}; R24-320, random weights\n")
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
