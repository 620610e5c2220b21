"""How well a checkpoint fits stored positions: the reference trainer's policy and value loss (azchess/training/train.py:436-549)
evaluated over rows of the shard store, without a trainer.  Forward and loss run on the device (M0Backend.score ->
m0_net_score, include/m0_score.h): per row 8 floats come back, never the 4672 logits.  This module is the plumbing around it:

    score_arrays(backend, s, pi, z, legal_mask, batch=N, **opts) -> f32 [N, 8]          # chunked M0Backend.score
    score_shards(data_dir, backend, sources=..., batch=N, per_sample=PATH, **opts) -> report

score_shards walks the store data_writer / npz_dataset define, in the order of its `shards` table, without shuffling and with
the partial last chunk of every shard.  A shard without `legal_mask` takes the reference's rule for itself (every row one-hot:
no masking; otherwise the support is pi > 0).  The report sums in float64 over all rows, per source and per shard: rows, the
means of policy loss, KL (policy loss - target entropy), value loss and total (policy + value, train.py:675), top-1/3/5 hit
rates of the target's best move, the mean soft-max mass on the support, the sign agreement of v with z over rows with z != 0,
and the count of each flag.  Rows with an empty support or non-finite network outputs are counted and left out of the means.

Command line: python -m matrix0_amd.score --config config.yaml --checkpoint A [--checkpoint B ...] --data DIR [--sources ...]
    [--batch N] [--json OUT] [--per-sample OUT.npz] [--label-smoothing X] [--value-loss mse|huber] [--huber-delta X]
label_smoothing, value_loss and huber_delta default to training.policy_label_smoothing, training.value_loss and
training.huber_delta of the config (the reference's keys).  One line per checkpoint; the exit status is 1 when any row had
non-finite outputs.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path
from typing import Dict, List, Optional, Sequence

import numpy as np

from ._abi import POLICY_SIZE, SCORE_COLS, SCORE_FLAGS
from .backend import NonFiniteScore, resolve_mask_mode
from .npz_dataset import ReplayReader

POLICY, ENTROPY, VALUE_LOSS, RANK, MASS, SUPPORT, VALUE, FLAGS = range(SCORE_COLS)
_LEFT_OUT = SCORE_FLAGS["empty"] | SCORE_FLAGS["nonfinite"]


def score_arrays(backend, s, pi, z, legal_mask=None, *, batch: int = 4096, mask_mode: Optional[str] = None, **opts) -> np.ndarray:
    """backend.score over the rows in chunks of `batch` (the last one partial): f32 [N, 8].  mask_mode None is resolved once,
    on the arrays given, not per chunk.  Rows of non-finite network outputs come back with flag 2 set; nothing is raised."""
    n = len(s)
    if batch <= 0:
        raise ValueError("batch must be positive")
    mode = resolve_mask_mode(pi, legal_mask, mask_mode)
    out = np.empty((n, SCORE_COLS), np.float32)
    for a in range(0, n, batch):
        b = min(n, a + batch)
        try:
            out[a:b] = backend.score(s[a:b], pi[a:b], z[a:b], None if legal_mask is None else legal_mask[a:b], mask_mode=mode, **opts)
        except NonFiniteScore as e:
            out[a:b] = e.rows
    return out


class Sums:
    """float64 sums of score columns; report() turns them into the means and rates of the module's docstring."""
    KEYS = ("policy_loss", "entropy", "value_loss", "top1", "top3", "top5", "support_mass", "sign_rows", "sign_agree")

    def __init__(self):
        self.rows = 0
        self.scored = 0
        self.flags = dict.fromkeys(SCORE_FLAGS, 0)
        self.sum = dict.fromkeys(self.KEYS, 0.0)

    def add(self, rows: np.ndarray, z: np.ndarray) -> None:
        r = np.asarray(rows, np.float64)
        flags = r[:, FLAGS].astype(np.int64)
        for name, bit in SCORE_FLAGS.items():
            self.flags[name] += int(((flags & bit) != 0).sum())
        keep = (flags & _LEFT_OUT) == 0
        r, zz = r[keep], np.asarray(z, np.float64).reshape(-1)[keep]
        self.rows += len(rows)
        self.scored += len(r)
        signed = zz != 0
        for key, x in (("policy_loss", r[:, POLICY]), ("entropy", r[:, ENTROPY]), ("value_loss", r[:, VALUE_LOSS]),
                       ("top1", r[:, RANK] < 1), ("top3", r[:, RANK] < 3), ("top5", r[:, RANK] < 5), ("support_mass", r[:, MASS]),
                       ("sign_rows", signed), ("sign_agree", signed & (np.sign(r[:, VALUE]) == np.sign(zz)))):
            self.sum[key] += float(np.sum(x, dtype=np.float64))

    def report(self) -> dict:
        n, s = self.scored, self.sum
        mean = lambda key: s[key] / n if n else None
        return {"rows": self.rows, "scored": n, "policy_loss": mean("policy_loss"),
                "kl": (s["policy_loss"] - s["entropy"]) / n if n else None, "value_loss": mean("value_loss"),
                "total": (s["policy_loss"] + s["value_loss"]) / n if n else None,
                "top1": mean("top1"), "top3": mean("top3"), "top5": mean("top5"), "support_mass": mean("support_mass"),
                "value_sign_agreement": s["sign_agree"] / s["sign_rows"] if s["sign_rows"] else None,
                "flags": dict(self.flags)}


def score_shards(data_dir, backend, *, sources: Sequence[str] = ("selfplay", ""), batch: int = 4096,
                 per_sample: Optional[str] = None, expected_planes: int = 19, **opts) -> dict:
    """The report over every readable shard of `data_dir` whose source is in `sources`: the overall figures, "by_source",
    "by_shard" (keyed by file name, in the table's order, each with its "mask_mode") and "skipped" (shards that do not load
    or do not hold 4672 columns; nothing is marked in the table -- this tool only reads).  per_sample=PATH also writes
    columns f32 [N, 8], shard_index i32 [N] into shards (file names) and row i32 [N], the row's index in its shard."""
    reader = ReplayReader(str(data_dir), expected_planes=expected_planes)
    total, by_source, by_shard, skipped = Sums(), {}, {}, []
    keep: Dict[str, List[np.ndarray]] = {"columns": [], "shard_index": [], "row": []}
    for path, _, source, corrupted in reader.index.rows():
        source = source or ""
        if corrupted or source not in sources or not Path(path).exists():
            continue
        try:
            got = reader._load(path)
        except Exception:
            got = None
        if got is None or got[1].shape[1] != POLICY_SIZE:          # the only policy layout the engine has
            skipped.append(Path(path).name)
            continue
        s, pi, z, mask = got
        mode = resolve_mask_mode(pi, mask, opts.get("mask_mode"))
        rows = score_arrays(backend, s, pi, z, mask, batch=batch, **dict(opts, mask_mode=mode))
        one = Sums()
        for sums in (total, by_source.setdefault(source, Sums()), one):
            sums.add(rows, z)
        by_shard[Path(path).name] = dict(one.report(), source=source, mask_mode=mode)
        if per_sample:
            keep["columns"].append(rows)
            keep["shard_index"].append(np.full(len(rows), len(by_shard) - 1, np.int32))
            keep["row"].append(np.arange(len(rows), dtype=np.int32))
    if per_sample:
        cat = lambda key, dtype, shape: np.concatenate(keep[key]) if keep[key] else np.zeros(shape, dtype)
        with open(per_sample, "wb") as f:
            np.savez(f, columns=cat("columns", np.float32, (0, SCORE_COLS)), shard_index=cat("shard_index", np.int32, (0,)),
                     row=cat("row", np.int32, (0,)), shards=np.array(list(by_shard), dtype=str))
    return dict(total.report(), by_source={k: v.report() for k, v in by_source.items()}, by_shard=by_shard, skipped=skipped)


def training_opts(cfg: dict, label_smoothing=None, value_loss=None, huber_delta=None) -> dict:
    """The loss settings of a run: `training.policy_label_smoothing`, `training.value_loss`, `training.huber_delta` of
    config.yaml (train.py:1308-1310, with its defaults); an argument that is not None overrides its key."""
    tr = cfg.get("training", {}) or {}
    return {"label_smoothing": float(tr.get("policy_label_smoothing", 0.0) if label_smoothing is None else label_smoothing),
            "value_loss": str(tr.get("value_loss", "mse") if value_loss is None else value_loss),
            "huber_delta": float(tr.get("huber_delta", 1.0) if huber_delta is None else huber_delta)}


def summary_line(name: str, r: dict) -> str:
    f = lambda x: "    n/a" if x is None else f"{x:7.4f}"
    return (f"{name}  rows {r['rows']} scored {r['scored']}  policy {f(r['policy_loss'])}  kl {f(r['kl'])}  value {f(r['value_loss'])}  "
            f"total {f(r['total'])}  top1 {f(r['top1'])}  top3 {f(r['top3'])}  top5 {f(r['top5'])}  mass {f(r['support_mass'])}  "
            f"sign {f(r['value_sign_agreement'])}  flags {r['flags']['empty']}/{r['flags']['nonfinite']}/{r['flags']['uniform']}")


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m matrix0_amd.score",
                                 description="Policy and value loss of checkpoints on stored positions, on one MI355X.")
    ap.add_argument("--config", required=True, help="config.yaml (or .json) of the run: model and training sections")
    ap.add_argument("--checkpoint", required=True, action="append", help="repeat to compare checkpoints side by side")
    ap.add_argument("--data", required=True, help="directory of the shard store (data_metadata.db and its shards)")
    ap.add_argument("--sources", nargs="*", default=["selfplay", ""], help="sources of the shards table to read")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--json", default=None, metavar="OUT", help="write {checkpoint: report} here")
    ap.add_argument("--per-sample", default=None, metavar="OUT.npz",
                    help="write the per-row columns (with several checkpoints: OUT.<k>.npz for checkpoint k)")
    ap.add_argument("--label-smoothing", type=float, default=None)
    ap.add_argument("--value-loss", choices=["mse", "huber"], default=None)
    ap.add_argument("--huber-delta", type=float, default=None)
    ap.add_argument("--device", type=int, default=0)
    return ap


def load_backend(model_cfg: dict, checkpoint: str, device: int):
    from .backend import M0Backend
    return M0Backend.from_checkpoint(model_cfg, checkpoint, device)


def main(argv: Optional[List[str]] = None) -> int:
    from .analysis import load_config
    args = build_parser().parse_args(argv)
    cfg = load_config(args.config)
    model_cfg = cfg.get("model", {}) or {}
    opts = training_opts(cfg, args.label_smoothing, args.value_loss, args.huber_delta)
    reports, nonfinite = {}, 0
    for k, ckpt in enumerate(args.checkpoint):
        per = args.per_sample
        if per and len(args.checkpoint) > 1:
            per = str(Path(per).with_suffix(f".{k}.npz"))
        be = load_backend(model_cfg, ckpt, args.device)
        try:
            r = score_shards(args.data, be, sources=tuple(args.sources), batch=args.batch, per_sample=per,
                             expected_planes=int(model_cfg.get("planes", 19)), **opts)
        finally:
            be.close()
        reports[ckpt] = r
        nonfinite += r["flags"]["nonfinite"]
        print(summary_line(ckpt, r), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"options": opts, "sources": list(args.sources), "checkpoints": reports}, f, indent=1)
    return 1 if nonfinite else 0


if __name__ == "__main__":
    sys.exit(main())
