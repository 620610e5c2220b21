"""A replay window resident on the device (include/m0_batch.h): packed rows (rowpack.py, about 160 bytes a row) are appended
shard by shard and stay in device memory; a batch names rows by id and one kernel launch writes them dense and already
transformed by the trainer's augmentation into device memory -- torch tensors for an unchanged trainer, or numpy arrays.  Only
the ids and kinds of a batch cross from the host.

    store = DeviceReplay.from_store("data", window_rows=1_000_000)          # every valid shard, oldest first
    for s, pi, z, legal_mask, ids, kind in store.batches(1024, epochs=1, torch=True):
        train_step(..., augment=False)                                       # the batch is already flipped or rotated

    store = DeviceReplay(device="host")                                      # the same calls on a machine without a GPU
    first = store.append(packed)                                             # range of the new rows' ids
    s, pi, z, legal_mask = store.batch(ids, kinds)                           # numpy
    s, pi, z, legal_mask, ssl, ssl_status = store.batch(ids, kinds, ssl=True)   # with the SSL target maps of s
    targets = ssl_targets(ssl)                                               # {"piece": [B,13,8,8], "threat": [B,8,8], ...}

    python -m matrix0_amd.device_replay info DIR

Row ids ascend over the life of a store and are never reused; evict(keep_rows) drops whole oldest shards."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
from pathlib import Path
from typing import Iterator, List, Optional, Sequence

import numpy as np

from . import _lib, rowpack
from ._abi import AUGMENT_KINDS, BATCH_SSL_CH, POLICY_SIZE, ROWSTORE_HOST, ROWSTORE_INFO
from .rowpack import DENSE_ROW_BYTES, PLANES, PackedRows

AUGMENT_MODES = ("trainer",) + tuple(AUGMENT_KINDS)


def trainer_kind(r: float, rotate180: bool = True) -> int:
    """The trainer's rule for one draw r in [0, 1) (train.py:282-295): r < 0.5 mirrors the files, r < 0.75 rotates by 180
    degrees when training.augment_rotate180 is set, otherwise the batch stays as it is."""
    if r < 0.5:
        return AUGMENT_KINDS["hflip"]
    if r < 0.75 and rotate180:
        return AUGMENT_KINDS["rot180"]
    return AUGMENT_KINDS["none"]


class DeviceReplay:
    def __init__(self, device=0, with_mask: bool = True):
        self.device = ROWSTORE_HOST if device == "host" else int(device)
        self.with_mask = bool(with_mask)
        self.skipped: List[str] = []
        self._L = _lib.lib()
        self._h = self._L.m0_rowstore_create(self.device, int(self.with_mask))
        if not self._h:
            raise RuntimeError(f"m0_rowstore_create failed: {_lib.last_error()}")

    # ---- life ----
    def close(self) -> None:
        if self._h:
            self._L.m0_rowstore_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- rows in, rows out ----
    def append(self, packed: PackedRows) -> range:
        """The rows as one more segment; the range of their ids.  ValueError, with the store unchanged, for arrays that do not
        hold together or whose masks are not the store's sort."""
        a = packed.c_arrays()
        first = C.c_int64(0)
        _lib.check(self._L.m0_rowstore_append(self._h, C.byref(a), C.byref(first)), "m0_rowstore_append")
        return range(first.value, first.value + packed.n)

    def append_shard(self, path) -> range:
        """A shard file: a packed one as it is, a dense one packed first (on the store's device, or on the CPU for a host store)."""
        packed, data = rowpack.read_shard(path, keys=rowpack.DENSE_KEYS)
        if packed is None:
            if not {"s", "pi", "z"} <= set(data):
                raise ValueError(f"{path}: no rows in it")
            n = len(data["s"])
            mask = np.asarray(data["legal_mask"]).reshape(n, -1) if "legal_mask" in data else None
            packed = rowpack.pack_rows(data["s"], data["pi"], np.asarray(data["z"]).reshape(-1), mask,
                                       device="host" if self.device == ROWSTORE_HOST else self.device)
        return self.append(packed)

    def evict(self, keep_rows: int) -> None:
        """Drops whole oldest segments while at least keep_rows rows stay; waits for the batches in flight first."""
        _lib.check(self._L.m0_rowstore_evict(self._h, int(keep_rows)), "m0_rowstore_evict")

    def info(self) -> dict:
        out = np.zeros(len(ROWSTORE_INFO), np.int64)
        _lib.check(self._L.m0_rowstore_info(self._h, _lib.ptr(out)), "m0_rowstore_info")
        return dict(zip(ROWSTORE_INFO, (int(x) for x in out)), dense_bytes=int(out[0]) * DENSE_ROW_BYTES)

    def resident_ids(self) -> np.ndarray:
        i = self.info()
        return np.arange(i["first_row"], i["next_row"], dtype=np.int64)

    @classmethod
    def from_store(cls, base_dir, sources: Sequence[str] = ("selfplay", ""), window_rows: Optional[int] = None, device=0,
                   with_mask: bool = True) -> "DeviceReplay":
        """Every valid shard of base_dir's table whose source is in `sources`, oldest first; then evicted down to window_rows.
        Shards that do not load, do not hold together or are not of the store's sort (with or without masks) are listed in
        .skipped by file name; nothing is marked in the table."""
        from .data_writer import ShardIndex
        store = cls(device, with_mask)
        for path, _, source, corrupted in ShardIndex(base_dir, create=False).rows():
            if corrupted or (source or "") not in sources or not Path(path).exists():
                continue
            try:
                store.append_shard(path)
            except Exception:
                store.skipped.append(Path(path).name)
        if window_rows is not None:
            store.evict(window_rows)
        return store

    # ---- batches ----
    def _ids_kinds(self, rows, kinds):
        rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        if kinds is not None:
            kinds = np.asarray(kinds)
            if kinds.ndim == 0:
                kinds = np.full(len(rows), int(kinds))
            if len(kinds) != len(rows) or (kinds < 0).any() or (kinds > 255).any():
                raise ValueError("kinds must hold one augmentation kind per row")
            kinds = np.ascontiguousarray(kinds, dtype=np.uint8)
        return rows, kinds

    def batch(self, rows, kinds=None, ssl: bool = False):
        """numpy (s f32 [B,19,8,8], pi f32 [B,4672], z f32 [B], legal_mask u8 [B,4672]) of the rows with these ids under these
        kinds (None: untransformed; one number: every row), or (s, pi, z) for a store without masks.  ssl=True appends the SSL
        target maps of s (ssl f32 [B,17,8,8]) and their status (ssl_status i32 [B]: 1 for a row whose planes give no targets,
        whose maps are zero), written by the same launch (include/m0_batch_ssl.h; ssl_targets splits the maps by task)."""
        rows, kinds = self._ids_kinds(rows, kinds)
        B = len(rows)
        s, pi, z = np.empty((B, PLANES, 8, 8), np.float32), np.empty((B, POLICY_SIZE), np.float32), np.empty(B, np.float32)
        mask = np.empty((B, POLICY_SIZE), np.uint8) if self.with_mask else None
        got = (s, pi, z, mask) if self.with_mask else (s, pi, z)
        if not ssl:
            _lib.check(self._L.m0_rowstore_batch(self._h, _lib.ptr(rows), _lib.ptr(kinds), B, _lib.ptr(s), _lib.ptr(pi), _lib.ptr(z),
                                                 _lib.ptr(mask), 0, None), "m0_rowstore_batch")
            return got
        maps, status = np.empty((B, BATCH_SSL_CH, 8, 8), np.float32), np.empty(B, np.int32)
        _lib.check(self._L.m0_rowstore_batch_ssl(self._h, _lib.ptr(rows), _lib.ptr(kinds), B, _lib.ptr(s), _lib.ptr(pi), _lib.ptr(z),
                                                 _lib.ptr(mask), _lib.ptr(maps), _lib.ptr(status), 0, None), "m0_rowstore_batch_ssl")
        return (*got, maps, status)

    def batch_torch(self, rows, kinds=None, out=None, ssl: bool = False):
        """The same batch as torch tensors on cuda:<device>, filled on torch's current stream without a wait: work enqueued on
        that stream afterwards sees them filled.  out: the tensors of an earlier call (with the same ssl), to be written again."""
        import torch
        if self.device == ROWSTORE_HOST:
            raise ValueError("a host store has no device tensors: use batch()")
        rows, kinds = self._ids_kinds(rows, kinds)
        B = len(rows)
        dev = torch.device("cuda", self.device)
        want = [((B, PLANES, 8, 8), torch.float32), ((B, POLICY_SIZE), torch.float32), ((B,), torch.float32)]
        if self.with_mask:
            want.append(((B, POLICY_SIZE), torch.uint8))
        if ssl:
            want += [((B, BATCH_SSL_CH, 8, 8), torch.float32), ((B,), torch.int32)]
        if out is None:
            out = tuple(torch.empty(shape, dtype=dtype, device=dev) for shape, dtype in want)
        out = tuple(out)
        if len(out) != len(want) or any(tuple(t.shape) != shape or t.dtype != dtype or t.device != dev or not t.is_contiguous()
                                        for t, (shape, dtype) in zip(out, want)):
            raise ValueError(f"out must be contiguous tensors on {dev} of {want}")
        ptrs = [C.c_void_p(t.data_ptr()) for t in out]
        if not self.with_mask:
            ptrs.insert(3, None)
        stream = torch.cuda.current_stream(dev).cuda_stream
        name = "m0_rowstore_batch_ssl" if ssl else "m0_rowstore_batch"
        _lib.check(getattr(self._L, name)(self._h, _lib.ptr(rows), _lib.ptr(kinds), B, *ptrs, 1, C.c_void_p(stream)), name)
        return out

    def plan(self, epoch: int, batch_size: int, seed: int = 0, augment: str = "trainer", rotate180: bool = True):
        """(ids i64 [batches, batch_size], kinds u8 [batches]) of one epoch over the rows resident now: a permutation of their ids
        from np.random.default_rng([seed, epoch]) cut into full batches (the tail is dropped), and one kind per batch -- with
        "trainer" from one draw per batch of the same generator (trainer_kind), otherwise the kind named."""
        if augment not in AUGMENT_MODES:
            raise ValueError(f"augment must be one of {AUGMENT_MODES}")
        rng = np.random.default_rng([int(seed), int(epoch)])
        ids = rng.permutation(self.resident_ids())
        n = len(ids) // int(batch_size)
        draws = rng.random(n)
        kinds = [trainer_kind(r, rotate180) if augment == "trainer" else AUGMENT_KINDS[augment] for r in draws]
        return ids[: n * int(batch_size)].reshape(n, int(batch_size)), np.array(kinds, np.uint8)

    def batches(self, batch_size: int, epochs: Optional[int] = None, seed: int = 0, augment: str = "trainer", rotate180: bool = True,
                torch: bool = False, ssl: bool = False) -> Iterator[tuple]:
        """Full batches, epoch after epoch (None: without end): (s, pi, z, legal_mask, ids, kind) -- without legal_mask for a store
        without masks, and with ssl=True (s, pi, z, legal_mask, ssl, ssl_status, ids, kind) -- as batch() or, with torch=True,
        batch_torch() gives them.  Batch j of epoch e is a function of (seed, e, j) and the resident rows alone (plan); ids and
        kind say what it holds, so a run can be replayed."""
        if int(batch_size) <= 0:
            raise ValueError("batch_size must be positive")
        epoch = 0
        while epochs is None or epoch < epochs:
            ids, kinds = self.plan(epoch, batch_size, seed, augment, rotate180)
            if len(ids) == 0:
                return
            for rows, kind in zip(ids, kinds):
                got = self.batch_torch(rows, int(kind), ssl=ssl) if torch else self.batch(rows, int(kind), ssl=ssl)
                yield (*got, rows, int(kind))
            epoch += 1


def ssl_targets(ssl) -> dict:
    """The maps of a batch (numpy array or torch tensor [B,17,8,8]) as the trainer's dictionary: piece [B,13,8,8], threat, pin, fork
    and control [B,8,8], views of `ssl` without a copy (_lib.split_ssl)."""
    if ssl.ndim != 4 or tuple(ssl.shape[1:]) != (BATCH_SSL_CH, 8, 8):
        raise ValueError(f"ssl must be [B,{BATCH_SSL_CH},8,8]")
    return _lib.split_ssl(ssl)


def info(base_dir, sources: Sequence[str] = ("selfplay", ""), window_rows: Optional[int] = None) -> dict:
    """What from_store would hold, counted on the CPU: rows, segments, packed bytes, RAW rows, the skipped shards, and the dense
    bytes those rows stand for."""
    with DeviceReplay.from_store(base_dir, sources, window_rows, device="host") as store:
        i = store.info()
        return {"rows": i["rows"], "segments": i["segments"], "packed_bytes": i["bytes"], "raw_rows": i["raw_rows"],
                "skipped": store.skipped, "dense_bytes": i["dense_bytes"]}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m matrix0_amd.device_replay", description=__doc__.split("\n\n")[0])
    ap.add_argument("command", choices=("info",))
    ap.add_argument("dir")
    ap.add_argument("--window-rows", type=int, default=None)
    a = ap.parse_args(argv)
    if not Path(a.dir).is_dir():
        ap.error(f"{a.dir} is not a directory")
    print(json.dumps(info(a.dir, window_rows=a.window_rows)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
