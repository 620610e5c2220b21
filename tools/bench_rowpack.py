#!/usr/bin/env python3
"""The measurements of the packed training rows (include/m0_rowpack.h), appended to profiles/rowpack.log:

  a  the pack and unpack kernels alone at B resident rows (m0_rowpack_bench: positions from seeded play, about 20 pi entries a row):
     microseconds per launch set and TB/s of the dense bytes read resp. written; beside them score_rows_kernel at the same B
     (m0_score_bench), the streaming kernel over the same arrays that serves as the yardstick
  b  M0Backend.score from host arrays, packed against dense, alternating after a warm-up (R24-320, random weights), with the
     bytes each call copies to the device
  c  score_shards over 8 192 rows in shards of 2 048, packed against dense shards, alternating
  d  import_pgn end to end over the fixture games, packed=True against dense, alternating
  e  bytes on disk per row of the same rows in both forms (np.savez_compressed either way), and in memory

The rows of b, c and e are the golden self-play rows of tests/golden/ref_worker_*.npz, tiled.  Each step runs as a child process
under its own time limit, and a step that fails ends the run.
`python tools/bench_rowpack.py [--batch 24576] [--log profiles/rowpack.log] [--commit TEXT] [--limit SECONDS]`"""
import argparse
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_score as bs          # noqa: E402  (the network and the options of the score's own measurements)


def rows(B):
    """B rows: the 375 golden self-play rows, tiled"""
    import numpy as np
    parts = [np.load(f) for f in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "ref_worker_*.npz")))]
    cat = lambda k: np.concatenate([d[k].reshape(len(d["s"]), *d[k].shape[1:]) for d in parts])
    idx = np.arange(B) % 375
    return (cat("s")[idx].astype(np.float32), cat("pi")[idx].astype(np.float32), cat("z").reshape(-1)[idx].astype(np.float32),
            cat("legal_mask").reshape(375, -1)[idx].astype(np.uint8))


def alternate(calls, n=3):
    """{name: best seconds of n} of the calls run in turn after one warm-up each"""
    for f in calls.values():
        f()
    best = {k: float("inf") for k in calls}
    for _ in range(n):
        for k, f in calls.items():
            t0 = time.perf_counter()
            f()
            best[k] = min(best[k], time.perf_counter() - t0)
    return best


def step_a(B):
    import ctypes as C
    from matrix0_amd import _lib
    L = _lib.lib()
    pack, unpack, nbytes = C.c_float(0), C.c_float(0), C.c_double(0)
    _lib.check(L.m0_rowpack_bench(0, B, 20, C.byref(pack), C.byref(unpack), C.byref(nbytes)), "m0_rowpack_bench")
    us, sbytes = C.c_float(0), C.c_double(0)
    _lib.check(L.m0_score_bench(0, B, 20, C.byref(us), C.byref(sbytes)), "m0_score_bench")
    tbs = lambda b, t: round(b / t / 1e6, 3)
    return {"B": B, "launches": 20, "dense_MB": round(nbytes.value / 1e6, 1),
            "pack": {"us": round(pack.value, 1), "TB_per_s_dense_read": tbs(nbytes.value, pack.value)},
            "unpack": {"us": round(unpack.value, 1), "TB_per_s_dense_written": tbs(nbytes.value, unpack.value)},
            "score_rows_kernel": {"us": round(us.value, 1), "TB_per_s": tbs(sbytes.value, us.value)}}


def step_b(B):
    from matrix0_amd import rowpack as rp
    be = bs.backend()
    s, pi, z, mask = rows(B)
    packed = rp.pack_rows(s, pi, z, mask, device=0)
    got = alternate({"dense": lambda: be.score(s, pi, z, mask, **bs.OPTS), "packed": lambda: be.score(packed=packed, **bs.OPTS)})
    same = bool((be.score(s, pi, z, mask, **bs.OPTS).view("u4") == be.score(packed=packed, **bs.OPTS).view("u4")).all())
    return {"B": B, "score_ms": {k: round(v * 1e3, 2) for k, v in got.items()}, "packed_over_dense": round(got["packed"] / got["dense"], 3),
            "rows_per_s": {k: round(B / v) for k, v in got.items()}, "forward_ms_device_resident": round(be.bench_forward(B, 3), 2),
            "MB_to_device": {"dense": round((s.nbytes + pi.nbytes + z.nbytes + mask.nbytes) / 1e6, 1), "packed": round(packed.nbytes / 1e6, 2)},
            "bitwise_equal": same}


def _store(base, n, shard):
    from matrix0_amd.data_writer import ShardIndex, write_npz
    s, pi, z, mask = rows(n)
    os.makedirs(os.path.join(base, "replays"))
    index = ShardIndex(base)
    for k, a in enumerate(range(0, n, shard)):
        path = os.path.join(base, "replays", f"replays_{k:03d}.npz")
        write_npz(path, dict(s=s[a:a + shard], pi=pi[a:a + shard], z=z[a:a + shard], legal_mask=mask[a:a + shard]))
        index.add(path, min(shard, n - a), "selfplay")


def _tree_bytes(base):
    return sum(os.path.getsize(os.path.join(d, f)) for d, _, fs in os.walk(base) for f in fs if f.endswith(".npz"))


def step_c(B):
    from pathlib import Path
    from matrix0_amd import rowpack as rp, score as sc
    be = bs.backend()
    n = 8192
    with tempfile.TemporaryDirectory() as tmp:
        _store(os.path.join(tmp, "dense"), n, 2048)
        rp._convert(Path(tmp, "dense"), Path(tmp, "packed"), True, 0)
        got = alternate({k: (lambda k=k: sc.score_shards(os.path.join(tmp, k), be, batch=4096, **bs.OPTS)) for k in ("dense", "packed")})
        same = sc.score_shards(os.path.join(tmp, "dense"), be, **bs.OPTS) == sc.score_shards(os.path.join(tmp, "packed"), be, **bs.OPTS)
    return {"rows": n, "score_shards_s": {k: round(v, 3) for k, v in got.items()}, "rows_per_s": {k: round(n / v) for k, v in got.items()},
            "packed_over_dense": round(got["packed"] / got["dense"], 3), "equal_reports": same}


def step_d(B):
    from matrix0_amd import game_import as gi
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from tests import replay_util as ru
    games = ru.fixture_games() * 4
    text = "\n".join(f'[Result "{res}"]\n\n' + " ".join(toks) + " " + res + "\n" for toks, res in games)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        def run(packed, k=[0]):
            k[0] += 1
            d = os.path.join(tmp, f"{packed}_{k[0]}")
            out["samples"] = gi.import_pgn(text, d, packed=packed)["samples"]
            out.setdefault("shard_bytes", {})["packed" if packed else "dense"] = _tree_bytes(d)
        got = alternate({"dense": lambda: run(False), "packed": lambda: run(True)})
    return {"games": len(games), "samples": out["samples"], "import_pgn_s": {k: round(v, 3) for k, v in got.items()},
            "samples_per_s": {k: round(out["samples"] / v) for k, v in got.items()},
            "packed_over_dense": round(got["packed"] / got["dense"], 3), "shard_bytes": out["shard_bytes"]}


def step_e(B):
    from pathlib import Path
    from matrix0_amd import rowpack as rp
    n = 8192
    with tempfile.TemporaryDirectory() as tmp:
        _store(os.path.join(tmp, "dense"), n, 2048)
        rp._convert(Path(tmp, "dense"), Path(tmp, "packed"), True, "host")
        disk = {k: _tree_bytes(os.path.join(tmp, k)) / n for k in ("dense", "packed")}
        info = rp.info(Path(tmp, "packed"))
    return {"rows": n, "disk_bytes_per_row": {k: round(v, 1) for k, v in disk.items()},
            "memory_bytes_per_row": {"dense": rp.DENSE_ROW_BYTES, "packed": round(info["packed_bytes_per_row"], 1)},
            "kinds": {"rows": info["rows_by_kind"], "masks": info["masks_by_kind"]}}


STEPS = {"a": ("pack and unpack kernels beside score_rows_kernel", step_a),
         "b": ("M0Backend.score from host arrays, packed against dense", step_b),
         "c": ("score_shards over 8192 rows, packed against dense shards", step_c),
         "d": ("import_pgn end to end, packed against dense", step_d),
         "e": ("bytes per row on disk and in memory", step_e)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=24576)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "rowpack.log"))
    ap.add_argument("--commit", default=None, help="what the header says was measured (default: git rev-parse --short HEAD)")
    ap.add_argument("--limit", type=int, default=300, help="seconds per step")
    ap.add_argument("--steps", default="".join(STEPS), help="the steps to run, e.g. ab")
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
        log.write(f"# tools/bench_rowpack.py --batch {args.batch}; commit {commit}; {time.strftime('%Y-%m-%d %H:%M:%S')}; "
                  f"options {json.dumps(bs.OPTS)}; R24-320, random weights\n")
        log.flush()
        for key in args.steps:
            what = STEPS[key][0]
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
