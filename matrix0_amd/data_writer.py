"""The shard store: the slice of DataManager the worker and the replay buffer use
(azchess/data_manager.py:198-243 _save_npz_shard / add_selfplay_data, :105-131 schema, :1622-1638 _record_shard).

Same on-disk contract: `<base>/selfplay/selfplay_<YYYYmmdd_HHMMSS>_<uuid8>.npz` written atomically
with np.savez_compressed, one row per shard in `<base>/data_metadata.db` table `shards`.  Three pieces carry it: write_npz (one
.npz, complete or absent), ShardIndex (the `shards` table; the only code that opens the database) and RowBuffer (per-game arrays
in, shards of an exact row count out).  The two writers below are built on them; game_import cuts and writes its shards with
RowBuffer and write_npz and records no row; npz_dataset.ReplayReader reads the table through ShardIndex."""
from __future__ import annotations

import hashlib
import os
import sqlite3
import tempfile
import time
import uuid
from contextlib import closing
from datetime import datetime
from pathlib import Path
from typing import Dict, List

import numpy as np

VERSION = "1.0.0"


def write_npz(path, arrays: Dict[str, np.ndarray]) -> None:
    """np.savez_compressed(path, **arrays) through a temp file beside it and os.replace: a reader never sees a partial shard.
    The temp name does not end in .npz (the stores are listed with *.npz).  Three attempts, as add_selfplay_data makes them."""
    path = Path(path)
    for attempt in range(3):
        try:
            with tempfile.NamedTemporaryFile(dir=str(path.parent), suffix=".npz.tmp", delete=False) as tf:
                np.savez_compressed(tf, **arrays)
            os.replace(tf.name, path)
            return
        except Exception:
            if attempt == 2:
                raise
            time.sleep(0.1 * (attempt + 1))


class ShardIndex:
    """The `shards` table of <base>/data_metadata.db (data_manager.py:105-131).  A writer creates the database and its two
    tables; a reader (create=False) leaves a directory without one as it is and sees no rows."""

    def __init__(self, base_dir, create: bool = True):
        self.db_path = Path(base_dir) / "data_metadata.db"
        if create:
            self._run("""CREATE TABLE IF NOT EXISTS shards (
                path TEXT PRIMARY KEY, size_bytes INTEGER, sample_count INTEGER, created_at TEXT, checksum TEXT,
                version TEXT, source TEXT, corrupted BOOLEAN DEFAULT FALSE, last_accessed TEXT)""")
            self._run("CREATE TABLE IF NOT EXISTS data_stats (key TEXT PRIMARY KEY, value TEXT, updated_at TEXT)")

    def _connect(self):
        conn = sqlite3.connect(self.db_path, timeout=30)
        conn.execute("PRAGMA journal_mode=WAL")
        conn.execute("PRAGMA synchronous=NORMAL")
        conn.execute("PRAGMA busy_timeout=30000")
        return conn

    def _run(self, sql: str, args=()) -> list:
        with closing(self._connect()) as conn:
            rows = conn.execute(sql, args).fetchall()
            conn.commit()
        return rows

    def add(self, path, sample_count: int, source: str) -> None:
        h = hashlib.sha256()
        with open(path, "rb") as f:
            for chunk in iter(lambda: f.read(1 << 20), b""):
                h.update(chunk)
        ts = datetime.now().strftime("%Y%m%d_%H%M%S")
        self._run("INSERT OR REPLACE INTO shards (path, size_bytes, sample_count, created_at, checksum, version, source, "
                  "last_accessed) VALUES (?, ?, ?, ?, ?, ?, ?, ?)",
                  (str(path), os.path.getsize(path), int(sample_count), ts, h.hexdigest(), VERSION, source, ts))

    def remove(self, path) -> None:
        self._run("DELETE FROM shards WHERE path = ?", (str(path),))

    def mark_corrupted(self, path) -> None:
        self._run("UPDATE shards SET corrupted = 1 WHERE path = ?", (str(path),))

    def rows(self) -> list:
        """(path, created_at, source, corrupted) per shard, in the order they were recorded."""
        if not self.db_path.exists():
            return []
        return self._run("SELECT path, created_at, source, corrupted FROM shards")


class RowBuffer:
    """Sample rows held as the parts they came in (one dict of equal-length arrays per game, the same keys in each); take(n)
    gives the oldest n rows (0 < n <= rows), splitting a part at the cut."""

    def __init__(self):
        self.parts: List[Dict[str, np.ndarray]] = []
        self.rows = 0

    def add(self, part: Dict[str, np.ndarray]) -> None:
        self.parts.append(part)
        self.rows += len(next(iter(part.values())))

    def take(self, n: int) -> Dict[str, np.ndarray]:
        got, need = [], n
        while need:
            part = self.parts.pop(0)
            if len(next(iter(part.values()))) > need:
                self.parts.insert(0, {key: a[need:] for key, a in part.items()})
                part = {key: a[:need] for key, a in part.items()}
            got.append(part)
            need -= len(next(iter(part.values())))
        self.rows -= n
        return {key: np.concatenate([p[key] for p in got]) for key in got[0]}


class SelfplayShardWriter:
    """packed=True writes every shard in the packed form of rowpack.py (packed on the CPU: the writer owns no device); the
    table's rows and everything else are as for dense shards, and ReplayReader reads either."""

    def __init__(self, base_dir: str = "data", packed: bool = False):
        self.base_dir = Path(base_dir)
        self.packed = bool(packed)
        self.selfplay_dir = self.base_dir / "selfplay"
        self.selfplay_dir.mkdir(parents=True, exist_ok=True)
        self.index = ShardIndex(self.base_dir)

    @staticmethod
    def validate_policy_targets(pi: np.ndarray) -> bool:
        """data_manager.py:1948-2007 (warn-only there): rows non-negative, finite, summing to 1 +- 0.01."""
        if pi.ndim != 2 or not np.all(np.isfinite(pi)) or np.any(pi < 0):
            return False
        return bool(np.all(np.abs(pi.sum(axis=1) - 1.0) <= 0.01))

    def _write_shard(self, data: Dict[str, np.ndarray], dir_path: Path) -> str:
        """<dir>/<dir name>_<timestamp>_<uuid8>.npz and its row (source "selfplay": the replay shards carry it too)."""
        ts = datetime.now().strftime("%Y%m%d_%H%M%S")
        path = dir_path / f"{dir_path.name}_{ts}_{uuid.uuid4().hex[:8]}.npz"
        rows = int(np.asarray(data["s"]).shape[0]) if "s" in data else 0
        if self.packed and rows:
            from .rowpack import pack_dict
            data = pack_dict(data, device="host")
        write_npz(path, data)
        self.index.add(path, rows, "selfplay")
        return str(path)

    def add_selfplay_data(self, data: Dict[str, np.ndarray], worker_id: int, game_id: int) -> str:
        return self._write_shard(data, self.selfplay_dir)


class ReplayShardWriter(SelfplayShardWriter):
    """Replay-buffer side of the same store: what `DataManager.compact_selfplay_to_replay`
    (azchess/data_manager.py:1378-1493) and `add_training_data` (:245-262) produce -- `<base>/replays/
    replays_<YYYYmmdd_HHMMSS>_<uuid8>.npz` shards of exactly `shard_size` samples (the tail shard is shorter) with keys
    `s f32[N,19,8,8]`, `pi f32[N,4672]`, `z f32[N]` and `legal_mask u8[N,4672]` when every game carried one, one row per
    shard in `shards` with source "selfplay", oldest replay shards pruned beyond `max_shards` (:1263-1293).

    Two ways in, same bytes out: `compact_selfplay_to_replay()` folds the per-game files of `<base>/selfplay/` in sorted
    name order (sources are moved to `<base>/backups/`, their rows dropped); `add_game()` takes finished games directly
    from the engine (no per-game file at all) -- call `close()` to flush the tail."""

    def __init__(self, base_dir: str = "data", max_shards: int = 128, shard_size: int = 16384, packed: bool = False):
        super().__init__(base_dir, packed=packed)
        self.replays_dir = self.base_dir / "replays"
        self.backups_dir = self.base_dir / "backups"
        self.replays_dir.mkdir(parents=True, exist_ok=True)
        self.backups_dir.mkdir(parents=True, exist_ok=True)
        self.max_shards = int(max_shards)
        self.shard_size = int(shard_size)
        self._buf = RowBuffer()
        self.summary = {"games": 0, "moves": 0, "resigned": 0, "draws": 0, "entropy": 0.0, "avg_sims": 0.0}
        self.written = []

    # -- intake ---------------------------------------------------------------------------------------------------
    def add_game(self, data: Dict[str, np.ndarray]) -> None:
        s, pi, z = np.asarray(data["s"]), np.asarray(data["pi"]), np.asarray(data["z"])
        if not (s.shape[0] == pi.shape[0] == z.shape[0]):
            raise ValueError("s / pi / z row counts differ")
        # legal_mask is decided per flushed shard: written iff every row of that shard came from a game that carried one
        # (the reference concatenates the masks of a shard's games or drops the key for that shard); until then a game
        # without one holds zeros, and `_has_mask` says which rows are which
        lm = data.get("legal_mask")
        have = lm is not None and np.asarray(lm).shape[0] == s.shape[0]
        self._buf.add({"s": s, "pi": pi, "z": z,
                       "legal_mask": (np.asarray(lm).reshape(s.shape[0], -1).astype(np.uint8, copy=False) if have
                                      else np.zeros((s.shape[0], pi.shape[1]), np.uint8)),
                       "_has_mask": np.full(s.shape[0], have, dtype=bool)})
        g = self.summary
        g["games"] += 1
        g["moves"] += int(np.asarray(data.get("meta_moves", [s.shape[0]])).reshape(-1)[0])
        g["resigned"] += int(np.asarray(data.get("meta_resigned", [0])).reshape(-1)[0])
        g["draws"] += int(np.asarray(data.get("meta_draw", [0])).reshape(-1)[0])
        g["entropy"] += float(np.asarray(data.get("meta_avg_policy_entropy", [0.0])).reshape(-1)[0])
        g["avg_sims"] += float(np.asarray(data.get("meta_avg_sims", [0.0])).reshape(-1)[0])
        while self._buf.rows >= self.shard_size:
            self._flush(self.shard_size)

    def close(self) -> None:
        if self._buf.rows > 0:
            self._flush(self._buf.rows)
        self.cleanup_old_shards(self.max_shards)

    # -- compaction of existing per-game files --------------------------------------------------------------------
    def compact_selfplay_to_replay(self) -> int:
        files = sorted(p for p in self.selfplay_dir.glob("*.npz") if p.is_file())
        for f in files:
            try:
                with np.load(f) as d:
                    game = {k: d[k] for k in d.files}
            except Exception:
                self.index.mark_corrupted(f)
                continue
            self.add_game(game)
            (self.backups_dir / f.name).write_bytes(f.read_bytes())
            f.unlink()
            self.index.remove(f)
        self.close()
        return len(files)

    # -- internals ------------------------------------------------------------------------------------------------
    def _flush(self, take: int) -> None:
        payload = self._buf.take(take)
        if not payload.pop("_has_mask").all():
            del payload["legal_mask"]
        self.written.append(self._write_shard(payload, self.replays_dir))

    def cleanup_old_shards(self, keep_recent: int) -> None:
        """Only replay shards under <base>/replays, never stockfish-tagged ones; newest `keep_recent` stay."""
        root = str(self.replays_dir.resolve())
        elig = [(p, c) for p, c, src, _ in self.index.rows()
                if str(Path(p).resolve()).startswith(root) and not (src or "").startswith("stockfish:")]
        elig.sort(key=lambda r: r[1], reverse=True)
        for p, _ in elig[keep_recent:]:
            Path(p).unlink(missing_ok=True)
            self.index.remove(p)
