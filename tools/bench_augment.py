#!/usr/bin/env python3
"""Two measurements of the trainer's augmentations on the device (include/m0_augment.h), appended to
profiles/augment.log:

  a  augment_rows_kernel alone at B rows on resident inputs (m0_augment_bench: 19 planes, with a mask, the three kinds in turn):
     microseconds per launch and GB/s over the bytes a launch must move, read and written; beside it score_rows_kernel at the same B
     (m0_score_bench), the streaming kernel over the same arrays that serves as the yardstick
  b  the wall time of score_arrays over the same B rows with augment=None, "hflip" and "trainer" (R24-320, random weights), and
     the forward alone (m0_net_bench_forward, resident input) at the same B

Each step runs as a child process under its own time limit, and a step that fails ends the run.
`python tools/bench_augment.py [--batch 4096] [--log profiles/augment.log] [--commit TEXT] [--limit SECONDS]`"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_score as bs          # noqa: E402  (the network, the options and the rows of the score's own measurements)


def step_a(B):
    import ctypes as C
    from matrix0_amd import _lib
    out = {"B": B, "launches": 20}
    for name, call in (("augment", _lib.lib().m0_augment_bench), ("score", _lib.lib().m0_score_bench)):
        us, nbytes = C.c_float(0), C.c_double(0)
        _lib.check(call(0, B, 20, C.byref(us), C.byref(nbytes)), name)
        gbs = nbytes.value / us.value / 1e3
        out[name] = {"us_per_launch": round(us.value, 1), "MB_per_launch": round(nbytes.value / 1e6, 1), "GB_per_s": round(gbs, 1),
                     "share_of_achievable_hbm": round(gbs / bs.HBM_ACHIEVABLE_GBS, 3)}
    out["augment_over_score_GB_per_s"] = round(out["augment"]["GB_per_s"] / out["score"]["GB_per_s"], 3)
    return out


def step_b(B):
    from matrix0_amd import score as sc
    be = bs.backend()
    x, pi, z, mask = bs.rows(B)
    ms, means = {}, {}
    for name, augment in (("none_given", None), ("hflip", "hflip"), ("trainer", "trainer")):
        sc.score_arrays(be, x, pi, z, mask, batch=B, augment=augment, **bs.OPTS)        # workspace, staging
        n = 3
        t0 = time.perf_counter()
        for _ in range(n):
            r = sc.score_arrays(be, x, pi, z, mask, batch=B, augment=augment, **bs.OPTS)
        ms[name] = (time.perf_counter() - t0) / n * 1e3
        means[name] = [round(float(v), 4) for v in r.reshape(-1, B, 8)[:, :, 0].mean(axis=1)]
    ms_fwd = be.bench_forward(B, 3)
    return {"B": B, "calls": 3, "score_arrays_ms": {k: round(v, 2) for k, v in ms.items()},
            "hflip_over_none_given": round(ms["hflip"] / ms["none_given"], 3),
            "trainer_over_none_given": round(ms["trainer"] / ms["none_given"], 3),
            "hflip_minus_none_given_over_forward": round((ms["hflip"] - ms["none_given"]) / ms_fwd, 4),
            "forward_ms_device_resident": round(ms_fwd, 2), "mean_policy_loss_per_kind": means}


STEPS = {"a": ("augment_rows_kernel beside score_rows_kernel", step_a),
         "b": ("score_arrays with augment None, hflip, trainer beside m0_net_bench_forward", step_b)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "augment.log"))
    ap.add_argument("--commit", default=None, help="what the header says was measured (default: git rev-parse --short HEAD)")
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
        log.write(f"# tools/bench_augment.py --batch {args.batch}; commit {commit}; {time.strftime('%Y-%m-%d %H:%M:%S')}; "
                  f"options {json.dumps(bs.OPTS)}; R24-320, random weights\n")
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
