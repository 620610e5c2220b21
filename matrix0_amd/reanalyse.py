"""Reanalyse: stored training rows searched again by the current network, their targets overwritten.

A shard (`s / pi / z / legal_mask`) cannot be improved once it is on disk: an imported game carries the one-hot `pi` of the
move a human played, an old self-play shard the visit counts of a network long replaced.  Here every stored row goes back
through the analysis engine: the planes are decoded to a position on the device (encoding.decode_planes says what they hold:
the men, side to move, cleaned castling rights and both clocks exactly; en passant from the row's legal mask; NO history),
searched at self-play throughput, and every root child's visit count comes back (AnalysisEngine.keep_visits).

Target rule
  pi2[row, policy_idx] = float32(visits / sum(visits))    the normalisation of the self-play record path (selfplay.hip
                                                          finish_search), so a reanalysed shard has the form of a fresh one
  z2 = (1 - value_mix) * z + value_mix * root_q           root_q is the root's q from the side to move's view (a backup adds the
                                                          leaf's value to the leaf and alternates the sign upward: the root
                                                          carries the value of the side to move there), which is z's
                                                          convention (z[i] = z_white * (+1 White to move, -1 Black)): no sign
                                                          flip.  Default value_mix = 0: z stays, bit for bit.
A row keeps its old pi and z when its planes do not decode (report: "decode:<reason>", mask mismatches included -- the audit
of the reference's audit_legal_masks.py), when its half-move plane is saturated (the clock was 99 OR MORE, the fifty- and
seventy-five-move tests of the search would start from a wrong clock; `search_saturated=True` searches it anyway), when the
root has no legal move, when the search overflowed its node arena or returned no visits.  A row answered from the endgame
tablebases takes the first line's move as a one-hot pi and the exact root_q as z.

Ids (the random streams' keys) default to the row's running index over the whole run: results do not depend on slots, shard
boundaries or batch size.

Command line: python -m matrix0_amd.reanalyse --config config.yaml --checkpoint CKPT --in DIR --out DIR --sims N
[--value-mix X] [--slots N] [--search-saturated] [--tablebase PATH [--tb-men N]]: reads every .npz under --in (sorted by
name), writes new shards under --out through the shard writer (never in place) and reanalyse_report.json beside them."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .encoding import DECODE_MASK_MISMATCH, DECODE_STATUS
from .rowpack import load_shard

_EPS = 1e-12
REPORT_NAME = "reanalyse_report.json"


def policy_from_visits(policy_idx, visits) -> Optional[Tuple[np.ndarray, np.ndarray]]:
    """(indices, float32 probabilities) of a policy target from a root's children, or None without a visit: each
    float32(double(n) / double(total)), as the self-play record path writes them."""
    idx = np.asarray(policy_idx, np.int64)
    n = np.asarray(visits, np.int64)
    total = int(n.sum())
    if idx.size == 0 or total <= 0:
        return None
    return idx, (n.astype(np.float64) / float(total)).astype(np.float32)


def blend_value(z: float, root_q: float, value_mix: float) -> np.float32:
    """z2 of the target rule; value_mix = 0 returns z itself."""
    if value_mix == 0.0:
        return np.float32(z)
    return np.float32((1.0 - float(value_mix)) * float(z) + float(value_mix) * float(root_q))


def _new_report() -> dict:
    return {"rows": 0, "searched": 0, "tablebase": 0, "kept": {}, "kept_ids": {}, "mask_mismatches": 0,
            "kl_sum": 0.0, "argmax_moved_rows": 0, "mean_kl": 0.0, "argmax_moved": 0.0}


def _finish_report(rep: dict) -> dict:
    changed = rep["searched"] + rep["tablebase"]
    rep["mean_kl"] = rep["kl_sum"] / changed if changed else 0.0
    rep["argmax_moved"] = rep["argmax_moved_rows"] / changed if changed else 0.0
    return rep


def merge_reports(reports: Sequence[dict]) -> dict:
    out = _new_report()
    for r in reports:
        for k in ("rows", "searched", "tablebase", "mask_mismatches", "kl_sum", "argmax_moved_rows"):
            out[k] += r[k]
        for reason, c in r["kept"].items():
            out["kept"][reason] = out["kept"].get(reason, 0) + c
        for reason, ids in r["kept_ids"].items():
            out["kept_ids"][reason] = (out["kept_ids"].get(reason, []) + list(ids))[:32]
    return _finish_report(out)


def reanalyse_arrays(s, pi, z, legal_mask=None, *, sims: int, value_mix: float = 0.0, ids=None, analyzer,
                     search_saturated: bool = False, batch_rows: int = 4096):
    """Search the rows of one shard again: s f32 [n,19,8,8], pi f32 [n,4672], z f32 [n], legal_mask [n,4672] or None (then en
    passant is unknown and no mask is audited) -> (pi2, z2, report).  `analyzer`: a matrix0_amd.analysis.Analyzer (or
    AnalyzerExt) whose engine searches; `ids`: one distinct id per row (default 0, 1, ...).  The inputs are not modified."""
    s = np.asarray(s)
    n = int(s.shape[0])
    pi = np.asarray(pi)
    z_in = np.asarray(z)
    if s.shape[1:] != (19, 8, 8) or pi.shape != (n, 4672) or z_in.size != n:
        raise ValueError("s must be [n,19,8,8], pi [n,4672], z [n]")
    if not 0.0 <= float(value_mix) <= 1.0:
        raise ValueError("value_mix must be in [0, 1]")
    if int(sims) < 1:
        raise ValueError("sims must be positive")
    if int(sims) > int(analyzer.cfg.num_simulations):
        raise ValueError(f"sims = {int(sims)} exceeds what the node arenas were sized for ({analyzer.cfg.num_simulations}): pass max_sims")
    mask = None if legal_mask is None else np.asarray(legal_mask).reshape(n, -1)
    ids = np.arange(n, dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)
    if ids.shape != (n,) or np.unique(ids).size != n:
        raise ValueError("ids must be distinct, one per row")
    pi2 = np.array(pi, dtype=np.float32, copy=True)
    z2 = np.array(z_in, dtype=np.float32, copy=True)
    zf = z2.reshape(-1)                                  # a view: z may be [n] or [n,1]
    rep = _new_report()
    rep["rows"] = n
    row_of = {int(i): r for r, i in enumerate(ids)}

    def keep(row: int, reason: str) -> None:
        rep["kept"][reason] = rep["kept"].get(reason, 0) + 1
        lst = rep["kept_ids"].setdefault(reason, [])
        if len(lst) < 32:
            lst.append(int(ids[row]))

    def changed(row: int) -> None:
        old = pi[row].astype(np.float64)
        new = pi2[row].astype(np.float64)
        rep["kl_sum"] += float(np.sum(old * (np.log(old + _EPS) - np.log(new + _EPS))))
        rep["argmax_moved_rows"] += int(int(np.argmax(old)) != int(np.argmax(new)))

    def take(r: dict) -> None:
        row = row_of[int(r["id"])]
        if r["status"] in ("checkmate", "stalemate"):
            keep(row, "no_legal_move")
        elif r["status"] == "tablebase":
            if not r["lines"]:
                keep(row, "no_visits")
                return
            pi2[row] = 0.0
            pi2[row, int(r["lines"][0]["policy_index"])] = 1.0
            zf[row] = np.float32(r["root_q"])
            rep["tablebase"] += 1
            changed(row)
        elif r["overflow"]:
            keep(row, "arena_overflow")
        else:
            target = policy_from_visits(r["policy_idx"], r["visits"])
            if target is None:
                keep(row, "no_visits")
                return
            pi2[row] = 0.0
            pi2[row, target[0]] = target[1]
            zf[row] = blend_value(zf[row], r["root_q"], value_mix)
            rep["searched"] += 1
            changed(row)

    engine = analyzer.engine
    engine.keep_visits(True)

    def drain() -> None:
        while True:
            r = engine.poll(visits=True)
            if r is None:
                return
            take(r)

    # a saturated half-move plane is exactly 1.0 on every square (a plane that varies does not decode at all)
    saturated = (s[:, 17, 0, 0] == np.float32(1.0)) if n else np.zeros(0, bool)
    low_water = 2 * int(engine.cfg.concurrent_games)
    for a in range(0, n, max(1, int(batch_rows))):
        rows = np.arange(a, min(n, a + max(1, int(batch_rows))))
        if not search_saturated:
            for row in rows[saturated[rows]]:
                keep(int(row), "halfmove_saturated")
            rows = rows[~saturated[rows]]
        if rows.size == 0:
            continue
        status, _ = engine.submit_planes(s[rows], None if mask is None else mask[rows], sims=int(sims), ids=ids[rows])
        for row, st in zip(rows, status):
            if st != 0:
                keep(int(row), "decode:" + DECODE_STATUS.get(int(st), str(int(st))))
                rep["mask_mismatches"] += int(int(st) == DECODE_MASK_MISMATCH)
        drain()
        while engine.pending() > low_water:
            analyzer._step()
            drain()
    while engine.pending() > 0:
        analyzer._step()
        drain()
    drain()
    return pi2, z2, _finish_report(rep)


def _shard_files(in_dir: Path, out_dir: Path) -> List[Path]:
    out = out_dir.resolve()
    return sorted((p for p in in_dir.rglob("*.npz") if p.is_file() and out not in p.resolve().parents),
                  key=lambda p: str(p.relative_to(in_dir)))


def reanalyse_shards(in_dir, out_dir, *, analyzer, sims: int, value_mix: float = 0.0, search_saturated: bool = False,
                     first_id: int = 0, batch_rows: int = 4096) -> dict:
    """Every .npz shard under `in_dir` (sorted by relative name) searched again and written as a new shard under `out_dir`
    by the shard writer (data_writer.SelfplayShardWriter: atomic file, a row in data_metadata.db); `s`, `legal_mask` and
    every other array of a shard are copied as they are, `pi` and `z` follow the target rule.  Never in place: `out_dir` must
    not be `in_dir`.  Row ids run on from `first_id` over the whole run.  Returns the report, also written as
    reanalyse_report.json under `out_dir`."""
    from .data_writer import SelfplayShardWriter
    in_dir, out_dir = Path(in_dir), Path(out_dir)
    if in_dir.resolve() == out_dir.resolve():
        raise ValueError("reanalyse never writes in place: out_dir must differ from in_dir")
    files = _shard_files(in_dir, out_dir)
    writer = SelfplayShardWriter(str(out_dir))
    next_id = int(first_id)
    reports, shards = [], []
    for k, f in enumerate(files):
        data = load_shard(f, device="host")                  # dense or packed (rowpack.py)
        if not {"s", "pi", "z"} <= set(data):
            shards.append({"source": str(f), "skipped": "no s / pi / z"})
            continue
        n = int(data["s"].shape[0])
        ids = np.arange(next_id, next_id + n, dtype=np.int64)
        next_id += n
        pi2, z2, rep = reanalyse_arrays(data["s"], data["pi"], data["z"], data.get("legal_mask"), sims=sims, value_mix=value_mix,
                                        ids=ids, analyzer=analyzer, search_saturated=search_saturated, batch_rows=batch_rows)
        out = dict(data)                                 # s, legal_mask and the rest: the very arrays that were read
        out["pi"], out["z"] = pi2, z2.astype(data["z"].dtype, copy=False).reshape(data["z"].shape)
        path = writer.add_selfplay_data(out, 0, k)
        reports.append(rep)
        shards.append({"source": str(f), "written": path, "first_id": int(ids[0]) if n else next_id, **rep})
    total = merge_reports(reports)
    total.update(sims=int(sims), value_mix=float(value_mix), search_saturated=bool(search_saturated), shards=shards)
    with open(out_dir / REPORT_NAME, "w") as fh:
        json.dump(total, fh, indent=1)
    return total


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m matrix0_amd.reanalyse",
                                 description="Search stored training shards again with a checkpoint on one MI355X.")
    ap.add_argument("--config", required=True, help="config.yaml (or .json) of the run: model, mcts sections")
    ap.add_argument("--checkpoint", required=True)
    ap.add_argument("--in", dest="in_dir", required=True, help="directory of .npz shards (read, never changed)")
    ap.add_argument("--out", dest="out_dir", required=True, help="directory the new shards and the report go to")
    ap.add_argument("--sims", type=int, default=None, help="simulations per row (default: the configured number)")
    ap.add_argument("--value-mix", type=float, default=0.0, help="z2 = (1 - x) * z + x * root_q (default 0: z stays)")
    ap.add_argument("--search-saturated", action="store_true", help="also search rows whose half-move plane is saturated")
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--tablebase", default=None, metavar="PATH", help="cache file of generated endgame tables")
    ap.add_argument("--tb-men", type=int, default=4)
    return ap


def main(argv: Optional[List[str]] = None) -> int:
    from . import analysis
    args = build_parser().parse_args(argv)
    cfg = analysis.load_config(args.config)
    from .backend import M0Backend
    be = M0Backend.from_checkpoint(cfg.get("model", {}) or {}, args.checkpoint, args.device)
    kw: Dict[str, object] = dict(slots=args.slots)
    if args.sims:
        kw["max_sims"] = args.sims
    if args.tablebase:
        kw.update(tablebase=args.tablebase, tb_men=args.tb_men)
    with analysis.Analyzer(be, cfg, **kw) as an:
        rep = reanalyse_shards(args.in_dir, args.out_dir, analyzer=an, sims=int(args.sims or an.cfg.num_simulations),
                               value_mix=args.value_mix, search_saturated=args.search_saturated)
    print(json.dumps({k: v for k, v in rep.items() if k != "shards"}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
