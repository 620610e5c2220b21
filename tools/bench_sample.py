#!/usr/bin/env python3
"""The measurements of the weighted row store (include/m0_batch_weighted.h), appended to
profiles/sample.log.  One device store of about a million resident rows -- the golden self-play rows packed once and appended
as 1024-row segments until a million are resident -- with gamma-distributed weights.  Per batch size B (1024 and 4096),
microseconds per call, device outputs, torch's current stream:

  a  sampled_batch     m0_rowstore_batch_sampled: the draw and the gather behind it
  b  planned_batch     m0_rowstore_batch with ids planned on the host (the path this library had before, untouched)
  c  draw              m0_rowstore_sample alone
  d  host_draw         what the device draw replaces when the weights change every batch: numpy cumulative sum over the window's
                       weights, searchsorted of B numbers, and the upload of the ids
  e  set_weights       m0_rowstore_set_weights of B device values at B device ids

Every figure is the wall time of `iters` calls and one synchronisation at the end, divided by iters, so it holds the host's share of
a call as a trainer's loop would see it; each is measured twice, the five alternating, and the spread of the two runs of one
figure is the noise floor.  What the header line says: (a) - (b), the price of drawing on the device, against (d).
`python tools/bench_sample.py [--log profiles/sample.log] [--commit TEXT] [--rows N] [--iters K]`"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

BATCHES = (1024, 4096)
SEGMENT = 1024


def build_store(rows):
    import numpy as np
    from matrix0_amd import device_replay as dr, rowpack as rp
    from tests import rowpack_cases as rc
    s, pi, z, mask = rc.worker_rows()
    take = np.arange(SEGMENT) % len(s)
    packed = rp.pack_rows(s[take], pi[take], z[take], mask[take], device="host")
    store = dr.DeviceReplay(0)
    while store.info()["rows"] < rows:
        store.append(packed)
    n = store.info()["rows"]
    w = np.random.default_rng(0).gamma(0.5, 2.0, n).astype(np.float32)
    store.set_weights(np.arange(n), w)
    return store, w


def timed(torch, iters, call):
    call(0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(iters):
        call(i + 1)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def measure(rows, iters):
    import numpy as np
    import torch
    store, w = build_store(rows)
    n = len(w)
    out = []
    for B in BATCHES:
        kinds = np.arange(B) % 3
        rng = np.random.default_rng(B)
        planned = [rng.integers(0, n, B) for _ in range(8)]
        tensors = store.batch_torch(planned[0], kinds)
        dev_ids = torch.from_numpy(planned[1]).cuda()
        dev_values = torch.rand(B, device="cuda")
        w64 = w.astype(np.float64)

        def host_draw(i):
            c = np.cumsum(w64)
            ids = np.searchsorted(c, rng.random(B) * c[-1], side="right")
            torch.from_numpy(ids).cuda()

        calls = {"sampled_batch": lambda i: store.sampled_batch(B, 1, i, kinds, torch=True, out=tensors),
                 "planned_batch": lambda i: store.batch_torch(planned[i % 8], kinds, out=tensors),
                 "draw": lambda i: store.sample(B, 1, i, torch=True),
                 "host_draw": host_draw,
                 "set_weights": lambda i: store.set_weights(dev_ids, dev_values)}
        us = {k: [] for k in calls}
        for _ in range(2):
            for k, call in calls.items():
                us[k].append(round(timed(torch, max(4, iters // 10) if k == "host_draw" else iters, call), 1))
        best = {k: min(v) for k, v in us.items()}
        noise = max(abs(v[0] - v[1]) for k, v in us.items() if k != "host_draw")
        out.append({"B": B, "resident_rows": n, "iters": iters, "us": us, "noise_floor_us": round(noise, 1),
                    "device_draw_price_us": round(best["sampled_batch"] - best["planned_batch"], 1),
                    "host_draw_us": best["host_draw"]})
    store.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "sample.log"))
    ap.add_argument("--commit", default=None, help="what the header says was measured (default: git rev-parse --short HEAD)")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    commit = args.commit
    if commit is None:
        got = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True)
        commit = got.stdout.strip() if got.returncode == 0 else "unknown"
    results = measure(args.rows, args.iters)
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "a") as log:
        log.write(f"# tools/bench_sample.py; commit {commit}; {time.strftime('%Y-%m-%d %H:%M:%S')}; (a) - (b) against (d), us per batch: "
                  + "; ".join(f"B={r['B']}: {r['device_draw_price_us']} against {r['host_draw_us']}" for r in results) + "\n")
        for r in results:
            line = json.dumps(r)
            log.write(line + "\n")
            print(line, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
