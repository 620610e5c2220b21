#!/usr/bin/env python3
"""Build time of the generated endgame tablebases on one GPU: the 3-man set, then the full 4-man set, with the number of
sweeps, the largest d and the milliseconds of every table.  Writes profiles/tablebase.log.

    python tools/bench_tablebase.py [--device 0] [--max-men 4] [--out profiles/tablebase.log]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--max-men", type=int, default=4, choices=(3, 4))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tablebase.log"))
    a = ap.parse_args()
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
