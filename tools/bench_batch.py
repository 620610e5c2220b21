#!/usr/bin/env python3
"""The measurements of the resident row store (include/m0_batch.h), appended to profiles/batch.log.  Per
batch size B (1024 and 4096):

  kernel  m0_rowstore_bench on resident seeded rows (those of m0_rowpack_bench, kinds 0, 1, 2 in turn): microseconds per batch
          of the fused kernel and of the chain it replaces on the same rows -- launch_encode_positions + launch_rowpack_unpack +
          launch_augment_rows -- alternating twice in one process; the spread between the two runs of each is the noise floor.
          GB/s of the dense bytes a batch writes, beside the HBM bandwidth a streaming kernel reaches on this part (6.3 TB/s).
  host    what the trainer does today: ReplayReader.get_training_batch over dense shards of the golden self-play rows, tiled,
          plus the upload of the batch (torch.from_numpy(...).to("cuda")), microseconds per batch over a few batches after one.

  ssl     (with --ssl) m0_rowstore_bench_ssl on the same rows: microseconds per batch of the launch that also writes the SSL target
          maps of the rows (include/m0_batch_ssl.h) and of what it replaces -- the launch without them, then the targets kernel of
          m0_ssl_targets_planes on the planes it wrote -- alternating twice; bytes per microsecond of what a batch writes, and the
          ratio of the launch with maps to the plain launch of the kernel step beside the ratio of the bytes written, 32 584 / 28 228.

The header of a run says the measured ratio chain / fused per B and whether it clears the noise floor.  Each step runs as a child
process under its own time limit, and a step that fails ends the run.
`python tools/bench_batch.py [--ssl] [--log profiles/batch.log] [--commit TEXT] [--limit SECONDS]`"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

BATCHES = (1024, 4096)
HBM_GB_PER_S = 6300.0


def step_kernel(B):
    import ctypes as C
    import numpy as np
    from matrix0_amd import _lib
    fused, chain, nbytes = np.zeros(2, np.float32), np.zeros(2, np.float32), C.c_double(0)
    _lib.check(_lib.lib().m0_rowstore_bench(0, B, 50, _lib.ptr(fused), _lib.ptr(chain), C.byref(nbytes)), "m0_rowstore_bench")
    f, c = float(fused.min()), float(chain.min())
    noise = max(abs(float(fused[0] - fused[1])), abs(float(chain[0] - chain[1])))
    gbs = lambda us: round(nbytes.value / us / 1e3, 1)
    return {"B": B, "launches": 50, "dense_MB": round(nbytes.value / 1e6, 1),
            "fused_us": [round(float(x), 1) for x in fused], "chain_us": [round(float(x), 1) for x in chain],
            "noise_floor_us": round(noise, 1), "chain_over_fused": round(c / f, 3), "faster_beyond_noise": bool(c - f > noise),
            "GB_per_s_dense_written": {"fused": gbs(f), "chain": gbs(c)}, "fraction_of_hbm": round(gbs(f) / HBM_GB_PER_S, 3)}


def step_ssl(B):
    import ctypes as C
    import numpy as np
    from matrix0_amd import _lib
    L = _lib.lib()
    fused, chain, nbytes = np.zeros(2, np.float32), np.zeros(2, np.float32), C.c_double(0)
    plain, plain_chain, plain_bytes = np.zeros(2, np.float32), np.zeros(2, np.float32), C.c_double(0)
    _lib.check(L.m0_rowstore_bench_ssl(0, B, 50, _lib.ptr(fused), _lib.ptr(chain), C.byref(nbytes)), "m0_rowstore_bench_ssl")
    _lib.check(L.m0_rowstore_bench(0, B, 50, _lib.ptr(plain), _lib.ptr(plain_chain), C.byref(plain_bytes)), "m0_rowstore_bench")
    f, c = float(fused.min()), float(chain.min())
    noise = max(abs(float(fused[0] - fused[1])), abs(float(chain[0] - chain[1])))
    per_us = lambda us: round(nbytes.value / us)
    return {"B": B, "launches": 50, "dense_MB": round(nbytes.value / 1e6, 1),
            "fused_us": [round(float(x), 1) for x in fused], "chain_us": [round(float(x), 1) for x in chain],
            "noise_floor_us": round(noise, 1), "chain_over_fused": round(c / f, 3), "faster_beyond_noise": bool(c - f > noise),
            "not_slower_beyond_noise": bool(f - c <= noise), "bytes_per_us_written": {"fused": per_us(f), "chain": per_us(c)},
            "plain_fused_us": [round(float(x), 1) for x in plain], "with_maps_over_plain": round(f / float(plain.min()), 3),
            "bytes_with_maps_over_plain": round(nbytes.value / plain_bytes.value, 3)}


def step_host(B):
    import torch
    from matrix0_amd.npz_dataset import ReplayReader
    import bench_rowpack as br
    n = 2 * B + 64
    with tempfile.TemporaryDirectory() as tmp:
        br._store(tmp, n, 2048)
        it = ReplayReader(tmp, seed=0).get_training_batch(B)
        upload = lambda batch: [torch.from_numpy(a).to("cuda") for a in batch]
        upload(next(it))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        count = 0
        for batch in it:
            upload(batch)
            count += 1
            if count == 4:
                break
        torch.cuda.synchronize()
        us = (time.perf_counter() - t0) / count * 1e6
    return {"B": B, "batches": count, "get_training_batch_plus_upload_us": round(us, 1)}


STEPS = {"kernel": ("fused kernel against the chain on resident rows", step_kernel),
         "host": ("ReplayReader.get_training_batch plus the upload", step_host)}
SSL_STEPS = {"ssl": ("launch with the SSL target maps against the plain launch plus the targets kernel", step_ssl)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "batch.log"))
    ap.add_argument("--commit", default=None, help="what the header says was measured (default: git rev-parse --short HEAD)")
    ap.add_argument("--limit", type=int, default=240, help="seconds per step")
    ap.add_argument("--ssl", action="store_true", help="also measure the launch that writes the SSL target maps")
    ap.add_argument("--step", choices=list(STEPS) + list(SSL_STEPS), default=None,
                    help="run one step in this process and print its JSON line")
    ap.add_argument("--batch", type=int, default=BATCHES[0])
    args = ap.parse_args()
    if args.step:
        print(json.dumps({**STEPS, **SSL_STEPS}[args.step][1](args.batch)), flush=True)
        return 0
    steps = {**STEPS, **SSL_STEPS} if args.ssl else STEPS
    commit = args.commit
    if commit is None:
        got = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True)
        commit = got.stdout.strip() if got.returncode == 0 else "unknown"
    lines, ratios, ssl_ratios, status = [], {}, {}, 0
    for B in BATCHES:
        for key, (what, _) in steps.items():
            try:
                got = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", key, "--batch", str(B)],
                                     capture_output=True, text=True, timeout=args.limit)
            except subprocess.TimeoutExpired:
                lines.append(f"{key} B={B} ({what}): no result within {args.limit} s; the run ends here")
                status = 1
                break
            if got.returncode != 0:
                lines.append(f"{key} B={B} ({what}): exit status {got.returncode}; the run ends here")
                sys.stderr.write(got.stderr[-2000:])
                status = 1
                break
            line = got.stdout.strip().splitlines()[-1]
            lines.append(f"{key} B={B} ({what}): {line}")
            print(key, B, line, flush=True)
            if key in ("kernel", "ssl"):
                r = json.loads(line)
                verdict = ("beyond" if r["faster_beyond_noise"] else
                           "fused SLOWER beyond" if not r.get("not_slower_beyond_noise", True) else "WITHIN")
                (ratios if key == "kernel" else ssl_ratios)[B] = (
                    f"{r['chain_over_fused']} ({verdict} the noise floor of {r['noise_floor_us']} us)")
        if status:
            break
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "a") as log:
        log.write(f"# tools/bench_batch.py; commit {commit}; {time.strftime('%Y-%m-%d %H:%M:%S')}; chain / fused per batch: "
                  + "; ".join(f"B={B}: {v}" for B, v in ratios.items())
                  + ("; with SSL maps, chain / fused per batch: " + "; ".join(f"B={B}: {v}" for B, v in ssl_ratios.items()) if args.ssl else "")
                  + "\n")
        for line in lines:
            log.write(line + "\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
