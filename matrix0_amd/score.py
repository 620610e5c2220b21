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
A packed shard (rowpack.py) is handed to M0Backend.score(packed=...) as it is and unpacked on the device -- the same columns and
the same report as for the dense shard; with ssl or augment it is unpacked on the host first.

Command line: python -m matrix0_amd.score --config config.yaml --checkpoint A [--checkpoint B ...] --data DIR [--sources ...]
    [--batch N] [--json OUT] [--per-sample OUT.npz] [--label-smoothing X] [--value-loss mse|huber] [--huber-delta X]
label_smoothing, value_loss and huber_delta default to training.policy_label_smoothing, training.value_loss and
training.huber_delta of the config (the reference's keys).  One line per checkpoint; the exit status is 1 when any row had
non-finite outputs.

The SSL term (ssl=..., --ssl): the reference's loss is policy + value + ssl_weight * ssl_loss (train.py:551-677), and with
ssl="auto" | "stored" | "planes" the same forward also scores the network's SSL heads (M0Backend.score_ssl -> m0_net_score_ssl,
include/m0_ssl_score.h; 16 more floats per row).  "stored" takes the targets the shard holds (ssl_piece [N,13,8,8], ssl_threat /
ssl_pin / ssl_fork / ssl_control [N,8,8]) and fails when a task of the network has no key; "planes" takes them from the stored
planes and ignores the shard's; "auto" decides per shard: stored when the shard has every key, otherwise planes.  Stored
targets are audited against the planes for free (flag "mismatch").  The report gains the key "ssl" (overall, per source, per
shard): `loss` per task, `ssl_total` = piece + sum of ssl_<task>_weight * loss over the network's tasks (resnet.py:990),
`total_with_ssl` = policy + value + ssl_weight * ssl_total, piece accuracy over all and over occupied squares, control accuracy,
precision and recall of threat and fork, and the flag counts.  The reference leaves a task out of ssl_total when its loss is not
finite or not > 0 (resnet.py:961-964, 988-996) PER TRAINING BATCH; here that rule is applied once, to the mean over the data set
(`dropped` names such tasks).  training.ssl_target_weight other than 1 scales one-hot targets during training and has no meaning
for a read-only score: it is refused.  Without ssl the report, the per-sample file and every call are what they were.
    [--ssl [auto|stored|planes]] [--ssl-weight X] [--ssl-task-weight task=X ...]
--ssl-weight defaults to training.ssl_weight (0.1 when absent, train.py:1306), a task's weight to model.ssl_<task>_weight (1).
With --per-sample the 16 SSL columns are written under the key `ssl_columns`.

The trainer's augmentations (augment=..., --augment): the reference's trainer (train.py:280-305, augment=True by default) draws one
r per batch and mirrors the files of s, pi and legal_mask when r < 0.5, rotates them by 180 degrees when 0.5 <= r < 0.75 and
training.augment_rotate180 holds (default true), and otherwise leaves them alone -- so what it optimises is mostly the loss on
transformed rows.  augment="none" | "hflip" | "rot180" scores every row under that kind (M0Backend.score(augment=...) ->
m0_net_score_aug, include/m0_augment.h: one upload, the transform on the device) and the report says which under "augment".
augment="trainer" scores every row under all three kinds (three forwards) and adds the block "augment" to the report, overall and
per shard: `by_kind` (the figures above for each kind), `weights` and `expected` = the policy loss, value loss and total the
trainer's draw gives in expectation, 0.5 hflip + 0.25 rot180 + 0.25 none, or 0.5 hflip + 0.5 none with
training.augment_rotate180: false (the elif chain of train.py:284-295), and `symmetry_gap`: the mean and the largest per-row
absolute difference of policy loss and value loss between "none" and "hflip", over the rows scored under both.  The figures
at the top of the report are then those of "none".  With --per-sample every kind's columns are written under
`columns_<kind>`.  The trainer leaves stored SSL targets untransformed, and targets taken from rotated planes are not positions the
decoder accepts: ssl together with an augmentation other than "none" is refused.  Without augment nothing changes.
    [--augment none|hflip|rot180|trainer]
"""
from __future__ import annotations

import argparse
import json
import sys
from collections import namedtuple
from pathlib import Path
from typing import Dict, List, Mapping, Optional, Sequence

import numpy as np

from ._abi import AUGMENT_KINDS, POLICY_SIZE, SCORE_COLS, SCORE_FLAGS, SSL_BITS, SSL_SCORE_COLS, SSL_SCORE_FLAGS
from .backend import NonFiniteScore, resolve_mask_mode
from .npz_dataset import ReplayReader

POLICY, ENTROPY, VALUE_LOSS, RANK, MASS, SUPPORT, VALUE, FLAGS = range(SCORE_COLS)
_LEFT_OUT = SCORE_FLAGS["empty"] | SCORE_FLAGS["nonfinite"]
SSL_MODES = ("auto", "stored", "planes")
SSL_TASKS = tuple(SSL_BITS)                      # the order of the heads and of a row's target maps
SSL_FLAGS_COL = SSL_SCORE_COLS - 1
AUGMENT_MODES = tuple(AUGMENT_KINDS) + ("trainer",)


def trainer_weights(augment_rotate180: bool = True) -> Dict[str, float]:
    """The share of batches the trainer's one draw r gives each kind (train.py:282-295): r < 0.5 mirrors, 0.5 <= r < 0.75 rotates
    when augment_rotate180, everything else stays."""
    rot = 0.25 if augment_rotate180 else 0.0
    return {"hflip": 0.5, "rot180": rot, "none": 0.5 - rot}


_SSL_AUG = "the trainer leaves stored SSL targets untransformed, and targets taken from rotated planes are not positions the decoder accepts"


def _check_augment(augment, ssl) -> None:
    if isinstance(augment, str) and augment not in AUGMENT_MODES:
        raise ValueError(f"augment must be one of {AUGMENT_MODES}, a per-row array of kinds or None, got {augment!r}")
    if ssl is not None and augment is not None and not (isinstance(augment, str) and augment == "none"):
        raise ValueError("ssl cannot be combined with an augmentation other than 'none': " + _SSL_AUG)
    if ssl is not None and ssl not in SSL_MODES:
        raise ValueError(f"ssl must be one of {SSL_MODES} or None, got {ssl!r}")


def _chunks(n: int, batch: int):
    """(a, b) of every chunk of `batch` rows out of n, the last one partial"""
    for a in range(0, n, batch):
        yield a, min(n, a + batch)


def pack_ssl_targets(arrays: Mapping[str, np.ndarray], n: int, tasks: Sequence[str]) -> np.ndarray:
    """A shard's ssl_piece [n,13,8,8] and ssl_threat / ssl_pin / ssl_fork / ssl_control [n,8,8] as f32 [n,17,64], the layout of
    m0_game_record.ssl.  KeyError when a task of `tasks` has no key; the map of a task that is not
    asked for and not stored stays zero."""
    out = np.zeros((n, 17, 64), np.float32)
    for k, t in enumerate(SSL_TASKS):
        a = arrays.get("ssl_" + t)
        if a is None:
            if t in tasks:
                raise KeyError(f"stored SSL targets lack ssl_{t}")
            continue
        a = np.asarray(a)
        if t == "piece":
            out[:, :13] = a.reshape(n, 13, 64)
        else:
            out[:, 12 + k] = a.reshape(n, 64)
    return out


def score_arrays(backend, s, pi, z, legal_mask=None, *, batch: int = 4096, mask_mode: Optional[str] = None,
                 ssl: Optional[str] = None, ssl_targets: Optional[np.ndarray] = None, augment=None, **opts):
    """backend.score over the rows in chunks of `batch` (the last one partial): f32 [N, 8].  mask_mode None is resolved once,
    on the arrays given, not per chunk.  Rows of non-finite network outputs come back with flag 2 set; nothing is raised.
    With ssl ("stored": ssl_targets f32 [N,17,64] as pack_ssl_targets makes them; "planes"; "auto": stored when targets are
    given) the chunks go through backend.score_ssl and the result is (f32 [N, 8], f32 [N, 16]).
    augment: None for the rows as they are (backend.score is called as ever); "none", "hflip", "rot180" or a per-row u8 [N] of
    AUGMENT_KINDS' values for the rows under that trainer augmentation (backend.score(augment=...)); "trainer" for all three,
    f32 [3, N, 8] in AUGMENT_KINDS' order.  With ssl only None and "none" are accepted."""
    n = len(s)
    if batch <= 0:
        raise ValueError("batch must be positive")
    _check_augment(augment, ssl)
    mode = resolve_mask_mode(pi, legal_mask, mask_mode)
    if isinstance(augment, str) and augment == "trainer":
        return np.stack([score_arrays(backend, s, pi, z, legal_mask, batch=batch, mask_mode=mode, augment=k, **opts)
                         for k in AUGMENT_KINDS])
    per_row = None if augment is None or isinstance(augment, str) else np.asarray(augment)
    if per_row is not None and per_row.shape != (n,):
        raise ValueError(f"per-row augmentation kinds must be [{n}], got {per_row.shape}")
    more = lambda a, b: {} if augment is None or ssl is not None else {"augment": augment if per_row is None else per_row[a:b]}
    cut = lambda x, a, b: None if x is None else x[a:b]
    if ssl == "stored" and ssl_targets is None:
        raise ValueError("ssl='stored' needs ssl_targets")
    targets = None if ssl == "planes" else ssl_targets
    outs = [np.empty((n, cols), np.float32) for cols in ((SCORE_COLS,) if ssl is None else (SCORE_COLS, SSL_SCORE_COLS))]
    for a, b in _chunks(n, batch):
        dense = (s[a:b], pi[a:b], z[a:b], cut(legal_mask, a, b))
        try:
            if ssl is None:
                got = (backend.score(*dense, mask_mode=mode, **opts, **more(a, b)),)
            else:
                got = backend.score_ssl(*dense, cut(targets, a, b), mask_mode=mode, **opts)
        except NonFiniteScore as e:
            got = (e.rows, e.ssl_rows)
        for out, rows in zip(outs, got):
            out[a:b] = rows
    return outs[0] if ssl is None else tuple(outs)


def _count_flags(sums, flags: np.ndarray, bits: Mapping[str, int], left_out: int) -> np.ndarray:
    """counts a batch's flags, rows and scored rows into a Sums or SslSums; returns the rows to sum: those with no flag of left_out"""
    for name, bit in bits.items():
        sums.flags[name] += int(((flags & bit) != 0).sum())
    keep = (flags & left_out) == 0
    sums.rows += len(flags)
    sums.scored += int(keep.sum())
    return keep


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
        keep = _count_flags(self, r[:, FLAGS].astype(np.int64), SCORE_FLAGS, _LEFT_OUT)
        r, zz = r[keep], np.asarray(z, np.float64).reshape(-1)[keep]
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


class SslSums:
    """float64 sums of SSL score columns (include/m0_ssl_score.h); report() turns them into the "ssl" block of the module's
    docstring.  Rows whose columns the kernel zeroed (non-finite heads; unusable planes without stored targets) are counted
    and left out."""

    def __init__(self):
        self.rows = 0
        self.scored = 0
        self.flags = dict.fromkeys(SSL_SCORE_FLAGS, 0)
        self.sum = np.zeros(SSL_FLAGS_COL, np.float64)

    def add(self, ssl_rows: np.ndarray, stored: bool) -> None:
        r = np.asarray(ssl_rows, np.float64)
        left_out = SSL_SCORE_FLAGS["nonfinite"] | (0 if stored else SSL_SCORE_FLAGS["planes"])
        keep = _count_flags(self, r[:, SSL_FLAGS_COL].astype(np.int64), SSL_SCORE_FLAGS, left_out)
        self.sum += r[keep, :SSL_FLAGS_COL].sum(axis=0, dtype=np.float64)

    def report(self, base: dict, tasks: Sequence[str], task_weights: Mapping[str, float], ssl_weight: float) -> dict:
        n, s = self.scored, self.sum
        ratio = lambda a, b: float(a / b) if b else None
        loss = {t: ratio(s[SSL_TASKS.index(t)], n) for t in tasks}
        counted = [t for t in tasks if loss[t] is not None and np.isfinite(loss[t]) and loss[t] > 0]
        ssl_total = float(sum((1.0 if t == "piece" else float(task_weights.get(t, 1.0))) * loss[t] for t in counted)) if n else None
        with_ssl = None
        if ssl_total is not None and base["policy_loss"] is not None:
            with_ssl = base["policy_loss"] + base["value_loss"] + float(ssl_weight) * ssl_total
        out = {"rows": self.rows, "scored": n, "tasks": list(tasks), "loss": loss, "dropped": [t for t in tasks if t not in counted],
               "ssl_total": ssl_total, "ssl_weight": float(ssl_weight), "total_with_ssl": with_ssl, "flags": dict(self.flags)}
        if "piece" in tasks:
            out["piece_accuracy"] = ratio(s[5], 64.0 * n)
            out["piece_accuracy_occupied"] = ratio(s[6], s[7])
        for t, c in (("threat", 8), ("fork", 11)):
            if t in tasks:
                out[t + "_precision"], out[t + "_recall"] = ratio(s[c], s[c + 1]), ratio(s[c], s[c + 2])
        if "control" in tasks:
            out["control_accuracy"] = ratio(s[14], 64.0 * n)
        return out


class AugmentSums:
    """Sums per kind of rows scored under all three, and of the per-row gap between "none" and "hflip"; report() gives the
    "augment" block of the module's docstring."""

    def __init__(self):
        self.kind = {k: Sums() for k in AUGMENT_KINDS}
        self.gap_rows = 0
        self.gap_sum = {"policy_loss": 0.0, "value_loss": 0.0}
        self.gap_max = {"policy_loss": 0.0, "value_loss": 0.0}

    def add(self, rows3: np.ndarray, z: np.ndarray) -> None:
        for k, rows in zip(AUGMENT_KINDS, rows3):
            self.kind[k].add(rows, z)
        a = np.asarray(rows3[AUGMENT_KINDS["none"]], np.float64)
        b = np.asarray(rows3[AUGMENT_KINDS["hflip"]], np.float64)
        both = ((a[:, FLAGS].astype(np.int64) | b[:, FLAGS].astype(np.int64)) & _LEFT_OUT) == 0
        self.gap_rows += int(both.sum())
        for key, col in (("policy_loss", POLICY), ("value_loss", VALUE_LOSS)):
            d = np.abs(a[both, col] - b[both, col])
            self.gap_sum[key] += float(d.sum(dtype=np.float64))
            if len(d):
                self.gap_max[key] = max(self.gap_max[key], float(d.max()))

    def report(self, weights: Mapping[str, float]) -> dict:
        by_kind = {k: v.report() for k, v in self.kind.items()}
        used = [k for k in AUGMENT_KINDS if weights[k] > 0]
        expected = {}
        for key in ("policy_loss", "value_loss", "total"):
            parts = [by_kind[k][key] for k in used]
            expected[key] = None if any(x is None for x in parts) else float(sum(weights[k] * x for k, x in zip(used, parts)))
        n = self.gap_rows
        gap = {key: {"mean": self.gap_sum[key] / n if n else None, "max": self.gap_max[key] if n else None}
               for key in ("policy_loss", "value_loss")}
        return {"mode": "trainer", "weights": {k: float(weights[k]) for k in AUGMENT_KINDS}, "by_kind": by_kind,
                "expected": expected, "symmetry_gap": dict(gap, rows=n)}


def _stored_ssl(path) -> Dict[str, np.ndarray]:
    with np.load(path) as d:
        return {k: d[k] for k in d.files if k.startswith("ssl_")}


def _packed_rows(path, expected_planes: int):
    """The rows of a packed shard (rowpack.py) that the reader would accept, still packed; None for any other file, of which
    nothing but the names in it is read here."""
    from . import rowpack
    try:
        packed, _ = rowpack.read_shard(path, keys=())
        if packed is not None:
            packed.validate()
    except Exception:
        return None
    if packed is None or expected_planes != rowpack.PLANES:
        return None
    finite = all(bool(np.isfinite(a).all()) for a in (packed.pi_val, packed.z, packed.raw_planes, packed.raw_pi))
    return packed if finite else None


def _score_packed(backend, packed, batch: int, **opts) -> np.ndarray:
    """score_arrays of packed rows: chunks of M0Backend.score(packed=...), unpacked on the device"""
    out = np.empty((packed.n, SCORE_COLS), np.float32)
    for a, b in _chunks(packed.n, batch):
        out[a:b] = backend.score(packed=packed.rows(a, b), **opts)
    return out


# _score_shard's answer; ssl_rows and stored (the targets were the shard's own) with ssl, rows3 (every kind's columns) with "trainer"
ShardScore = namedtuple("ShardScore", "rows z mode ssl_rows stored rows3", defaults=(None, False, None))


def _score_shard(backend, reader, path, batch, expected_planes, ssl, tasks, augment, opts) -> Optional[ShardScore]:
    """One shard scored as score_shards was asked to; None when it does not load, does not hold 4672 columns or, packed, does not
    hold together.  A packed shard goes to the device as it is when nothing but the rows' own columns is wanted."""
    packed = _packed_rows(path, expected_planes) if ssl is None and augment is None else None
    if packed is not None:
        from .rowpack import mask_mode_of
        mode = mask_mode_of(packed, opts.get("mask_mode"))
        try:
            return ShardScore(_score_packed(backend, packed, batch, **dict(opts, mask_mode=mode)), packed.z, mode)
        except NonFiniteScore:
            raise
        except ValueError:                                          # as an unreadable dense shard
            return None
    try:
        s, pi, z, mask = reader._load(path)                         # None for a shard the reader refuses: that fails here as well
    except Exception:
        return None
    if pi.shape[1] != POLICY_SIZE:                                  # the only policy layout the engine has
        return None
    mode = resolve_mask_mode(pi, mask, opts.get("mask_mode"))
    opts = dict(opts, mask_mode=mode)
    if ssl is None:
        rows = score_arrays(backend, s, pi, z, mask, batch=batch, augment=augment, **opts)
        return ShardScore(rows[AUGMENT_KINDS["none"]], z, mode, rows3=rows) if augment == "trainer" else ShardScore(rows, z, mode)
    have = {} if ssl == "planes" else _stored_ssl(path)
    stored = ssl == "stored" or (ssl == "auto" and all("ssl_" + t in have for t in tasks))
    try:
        targets = pack_ssl_targets(have, len(s), tasks) if stored else None
    except KeyError as e:
        raise KeyError(f"{Path(path).name}: {e.args[0]} (ssl='stored')") from None
    rows, ssl_rows = score_arrays(backend, s, pi, z, mask, batch=batch, ssl="stored" if stored else "planes", ssl_targets=targets, **opts)
    return ShardScore(rows, z, mode, ssl_rows, stored)


def _write_per_sample(path, kept: Sequence[ShardScore], shards: Sequence[str], ssl: Optional[str], augment: Optional[str]) -> None:
    """The per-row columns of every scored shard, in the order of `shards`, as the .npz of score_shards' docstring."""
    cat = lambda parts, dtype=np.float32, shape=(0, SCORE_COLS): np.concatenate(parts) if parts else np.zeros(shape, dtype)
    more = {} if ssl is None else {"ssl_columns": cat([x.ssl_rows for x in kept], np.float32, (0, SSL_SCORE_COLS))}
    for k in (AUGMENT_KINDS if augment == "trainer" else () if augment is None else (augment,)):
        more["columns_" + k] = cat([x.rows3[AUGMENT_KINDS[k]] if augment == "trainer" else x.rows for x in kept])
    with open(path, "wb") as f:
        np.savez(f, columns=cat([x.rows for x in kept]),
                 shard_index=cat([np.full(len(x.rows), i, np.int32) for i, x in enumerate(kept)], np.int32, (0,)),
                 row=cat([np.arange(len(x.rows), dtype=np.int32) for x in kept], np.int32, (0,)),
                 shards=np.array(list(shards), dtype=str), **more)


def score_shards(data_dir, backend, *, sources: Sequence[str] = ("selfplay", ""), batch: int = 4096,
                 per_sample: Optional[str] = None, expected_planes: int = 19, ssl: Optional[str] = None,
                 ssl_weight: float = 0.1, ssl_task_weights: Optional[Mapping[str, float]] = None,
                 ssl_target_weight: float = 1.0, augment: Optional[str] = None, augment_rotate180: bool = True, **opts) -> dict:
    """The report over every readable shard of `data_dir` whose source is in `sources`: the overall figures, "by_source",
    "by_shard" (keyed by file name, in the table's order, each with its "mask_mode") and "skipped" (shards that do not load
    or do not hold 4672 columns; nothing is marked in the table -- this tool only reads).  per_sample=PATH also writes
    columns f32 [N, 8], shard_index i32 [N] into shards (file names) and row i32 [N], the row's index in its shard.
    ssl="auto" | "stored" | "planes" adds the "ssl" blocks of the module's docstring (a shard's also says its "targets":
    "stored" or "planes") and ssl_columns f32 [N, 16] to the per-sample file; ssl_weight is training.ssl_weight (its default
    there is 0.1, train.py:1306), ssl_task_weights {task: weight} defaults to backend.model_cfg's ssl_<task>_weight.  ssl=None
    adds nothing.  augment="none" | "hflip" | "rot180" scores the rows under that trainer augmentation and names it under
    "augment"; augment="trainer" scores them under all three and adds the "augment" block of the module's docstring (overall and
    per shard), weighted by trainer_weights(augment_rotate180); the per-sample file gains columns_<kind>.  augment=None adds
    nothing."""
    if augment is not None and not isinstance(augment, str):
        raise ValueError("score_shards takes an augmentation by name")
    _check_augment(augment, ssl)
    trainer = augment == "trainer"
    weights = trainer_weights(augment_rotate180)
    tasks: List[str] = []
    if ssl is not None:
        if float(ssl_target_weight) != 1.0:
            raise ValueError("ssl_target_weight other than 1.0 scales the targets of a training step; a read-only score has no use for it")
        tasks = list(backend.ssl_tasks)
        if not tasks:
            raise ValueError("the network has no SSL heads to score")
        if ssl_task_weights is None:
            model_cfg = getattr(backend, "model_cfg", {}) or {}
            ssl_task_weights = {t: float(model_cfg.get(f"ssl_{t}_weight", 1.0)) for t in tasks}
        ssl_report = lambda sums, base: sums.report(base, tasks, ssl_task_weights, ssl_weight)
    reader = ReplayReader(str(data_dir), expected_planes=expected_planes)
    total, by_source, by_shard, skipped = Sums(), {}, {}, []
    ssl_total, ssl_by_source, aug_total, kept = SslSums(), {}, AugmentSums(), []
    for path, _, source, corrupted in reader.index.rows():
        source = source or ""
        if corrupted or source not in sources or not Path(path).exists():
            continue
        name = Path(path).name
        got = _score_shard(backend, reader, path, batch, expected_planes, ssl, tasks, augment, opts)
        if got is None:
            skipped.append(name)
            continue
        one = Sums()
        for sums in (total, by_source.setdefault(source, Sums()), one):
            sums.add(got.rows, got.z)
        by_shard[name] = dict(one.report(), source=source, mask_mode=got.mode)
        if trainer:
            aug_one = AugmentSums()
            for sums in (aug_total, aug_one):
                sums.add(got.rows3, got.z)
            by_shard[name]["augment"] = aug_one.report(weights)
        if ssl is not None:
            ssl_one = SslSums()
            for sums in (ssl_total, ssl_by_source.setdefault(source, SslSums()), ssl_one):
                sums.add(got.ssl_rows, got.stored)
            by_shard[name]["ssl"] = dict(ssl_report(ssl_one, one.report()), targets="stored" if got.stored else "planes")
        if per_sample:
            kept.append(got)
    if per_sample:
        _write_per_sample(per_sample, kept, by_shard, ssl, augment)
    report = dict(total.report(), by_source={k: v.report() for k, v in by_source.items()}, by_shard=by_shard, skipped=skipped)
    if trainer:
        report["augment"] = aug_total.report(weights)
    elif augment is not None:
        report["augment"] = {"mode": augment}
    if ssl is not None:
        report["ssl"] = ssl_report(ssl_total, report)
        for k, v in ssl_by_source.items():
            report["by_source"][k]["ssl"] = ssl_report(v, report["by_source"][k])
    return report


def training_opts(cfg: dict, label_smoothing=None, value_loss=None, huber_delta=None) -> dict:
    """The loss settings of a run: `training.policy_label_smoothing`, `training.value_loss`, `training.huber_delta` of
    config.yaml (train.py:1308-1310, with its defaults); an argument that is not None overrides its key."""
    tr = cfg.get("training", {}) or {}
    return {"label_smoothing": float(tr.get("policy_label_smoothing", 0.0) if label_smoothing is None else label_smoothing),
            "value_loss": str(tr.get("value_loss", "mse") if value_loss is None else value_loss),
            "huber_delta": float(tr.get("huber_delta", 1.0) if huber_delta is None else huber_delta)}


def ssl_opts(cfg: dict, tasks: Sequence[str] = SSL_TASKS, ssl_weight=None, task_weights: Optional[Mapping[str, float]] = None) -> dict:
    """The SSL settings of a run: `training.ssl_weight` (train.py:1306, 0.1 when absent), `model.ssl_<task>_weight`
    (resnet.py:990, 1 when absent) and `training.ssl_target_weight`; the arguments override the keys."""
    tr, model = cfg.get("training", {}) or {}, cfg.get("model", {}) or {}
    weights = {t: float(model.get(f"ssl_{t}_weight", 1.0)) for t in tasks if t != "piece"}
    for t, w in (task_weights or {}).items():
        if t not in weights:
            raise ValueError(f"no SSL task weight for {t!r}: the weighted tasks are {sorted(weights)}")
        weights[t] = float(w)
    return {"ssl_weight": float(tr.get("ssl_weight", 0.1) if ssl_weight is None else ssl_weight), "ssl_task_weights": weights,
            "ssl_target_weight": float(tr.get("ssl_target_weight", 1.0))}


_f = lambda x: "    n/a" if x is None else f"{x:7.4f}"              # a figure of the summary lines


def ssl_summary_line(name: str, r: dict) -> str:
    x = r["ssl"]
    losses = "  ".join(f"{t} {_f(v)}" for t, v in x["loss"].items())
    return (f"{name}  ssl rows {x['rows']} scored {x['scored']}  {losses}  ssl_total {_f(x['ssl_total'])}  "
            f"total_with_ssl {_f(x['total_with_ssl'])} (ssl_weight {x['ssl_weight']:g})  piece acc {_f(x.get('piece_accuracy'))} "
            f"occupied {_f(x.get('piece_accuracy_occupied'))}  control acc {_f(x.get('control_accuracy'))}  "
            f"flags {x['flags']['planes']}/{x['flags']['nonfinite']}/{x['flags']['mismatch']}")


def augment_summary_line(name: str, r: dict) -> str:
    x = r["augment"]
    if x["mode"] != "trainer":
        return f"{name}  augment {x['mode']}: the figures above are those of the rows under it"
    kinds = "  ".join(f"{k} policy {_f(v['policy_loss'])} value {_f(v['value_loss'])} total {_f(v['total'])}" for k, v in x["by_kind"].items())
    w, e, g = x["weights"], x["expected"], x["symmetry_gap"]
    return (f"{name}  augment trainer  {kinds}  expected ({w['hflip']:g} hflip + {w['rot180']:g} rot180 + {w['none']:g} none) "
            f"policy {_f(e['policy_loss'])} value {_f(e['value_loss'])} total {_f(e['total'])}  symmetry gap none/hflip over {g['rows']} rows: "
            f"policy mean {_f(g['policy_loss']['mean'])} max {_f(g['policy_loss']['max'])}  value mean {_f(g['value_loss']['mean'])} "
            f"max {_f(g['value_loss']['max'])}")


def summary_line(name: str, r: dict) -> str:
    return (f"{name}  rows {r['rows']} scored {r['scored']}  policy {_f(r['policy_loss'])}  kl {_f(r['kl'])}  value {_f(r['value_loss'])}  "
            f"total {_f(r['total'])}  top1 {_f(r['top1'])}  top3 {_f(r['top3'])}  top5 {_f(r['top5'])}  mass {_f(r['support_mass'])}  "
            f"sign {_f(r['value_sign_agreement'])}  flags {r['flags']['empty']}/{r['flags']['nonfinite']}/{r['flags']['uniform']}")


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
    ap.add_argument("--ssl", nargs="?", const="auto", default=None, choices=list(SSL_MODES),
                    help="also score the SSL heads: targets as stored, from the planes, or per shard (auto, the default of --ssl)")
    ap.add_argument("--ssl-weight", type=float, default=None, help="overrides training.ssl_weight")
    ap.add_argument("--ssl-task-weight", action="append", default=[], metavar="TASK=X", help="overrides model.ssl_<task>_weight")
    ap.add_argument("--augment", default=None, choices=list(AUGMENT_MODES),
                    help="score the rows under a trainer augmentation; trainer: under all three, with the loss the trainer's draw "
                         "expects (training.augment_rotate180 of the config decides the weights) and the none/hflip symmetry gap")
    ap.add_argument("--device", type=int, default=0)
    return ap


def load_backend(model_cfg: dict, checkpoint: str, device: int):
    from .backend import M0Backend
    return M0Backend.from_checkpoint(model_cfg, checkpoint, device)


def main(argv: Optional[List[str]] = None) -> int:
    from .analysis import load_config
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.ssl and args.augment not in (None, "none"):
        parser.error("--ssl cannot be combined with --augment other than none: " + _SSL_AUG)
    cfg = load_config(args.config)
    model_cfg = cfg.get("model", {}) or {}
    opts = training_opts(cfg, args.label_smoothing, args.value_loss, args.huber_delta)
    more = {}
    if args.ssl:
        pairs = [w.partition("=") for w in args.ssl_task_weight]
        more = dict(ssl_opts(cfg, ssl_weight=args.ssl_weight, task_weights={t: float(x) for t, _, x in pairs}), ssl=args.ssl)
    aug = {}
    if args.augment:
        aug = {"augment": args.augment, "augment_rotate180": bool((cfg.get("training", {}) or {}).get("augment_rotate180", True))}
    reports, nonfinite = {}, 0
    for k, ckpt in enumerate(args.checkpoint):
        per = args.per_sample
        if per and len(args.checkpoint) > 1:
            per = str(Path(per).with_suffix(f".{k}.npz"))
        be = load_backend(model_cfg, ckpt, args.device)
        try:
            r = score_shards(args.data, be, sources=tuple(args.sources), batch=args.batch, per_sample=per,
                             expected_planes=int(model_cfg.get("planes", 19)), **opts, **more, **aug)
        finally:
            be.close()
        reports[ckpt] = r
        nonfinite += r["flags"]["nonfinite"]
        print(summary_line(ckpt, r), flush=True)
        if args.ssl:
            nonfinite += r["ssl"]["flags"]["nonfinite"]
            print(ssl_summary_line(ckpt, r), flush=True)
        if args.augment:
            if args.augment == "trainer":
                nonfinite += sum(v["flags"]["nonfinite"] for k, v in r["augment"]["by_kind"].items() if k != "none")
            print(augment_summary_line(ckpt, r), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict({"options": opts, "sources": list(args.sources), "checkpoints": reports},
                           **({"ssl_options": more} if args.ssl else {}), **({"augment_options": aug} if args.augment else {})),
                      f, indent=1)
    return 1 if nonfinite else 0


if __name__ == "__main__":
    sys.exit(main())
