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
from ._abi import (AUGMENT_KINDS, BATCH_SSL_CH, POLICY_SIZE, ROWSTORE_HOST, ROWSTORE_INFO, SCORE_COLS, WEIGHT_MAX, WEIGHTS_INFO,
                   WeightRule)
from .rowpack import DENSE_ROW_BYTES, PLANES, PackedRows

AUGMENT_MODES = ("trainer",) + tuple(AUGMENT_KINDS)
U64 = (1 << 64) - 1


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
                torch: bool = False, ssl: bool = False, weighted: bool = False, stratified: bool = False) -> Iterator[tuple]:
        """Full batches, epoch after epoch (None: without end): (s, pi, z, legal_mask, ids, kind) -- without legal_mask for a store
        without masks, and with ssl=True (s, pi, z, legal_mask, ssl, ssl_status, ids, kind) -- as batch() or, with torch=True,
        batch_torch() gives them.  Batch j of epoch e is a function of (seed, e, j) and the resident rows alone (plan); ids and
        kind say what it holds, so a run can be replayed.

        weighted=True draws the rows in proportion to their weights instead (sampled_batch): an epoch is resident // batch_size
        batches, batch j of epoch e is draw (e << 32) | j under `seed` with the kind plan's generator gives it, and the tuple
        gains prob behind kind: (..., ids, kind, prob).  It is a function of (seed, e, j), the resident rows and their weights."""
        if int(batch_size) <= 0:
            raise ValueError("batch_size must be positive")
        epoch = 0
        while epochs is None or epoch < epochs:
            if weighted:
                kinds = self.plan(epoch, batch_size, seed, augment, rotate180)[1]
                if len(kinds) == 0:
                    return
                for j, kind in enumerate(kinds):
                    *got, rows, prob = self.sampled_batch(batch_size, seed, (epoch << 32) | j, int(kind), stratified, ssl, torch)
                    yield (*got, rows, int(kind), prob)
                epoch += 1
                continue
            ids, kinds = self.plan(epoch, batch_size, seed, augment, rotate180)
            if len(ids) == 0:
                return
            for rows, kind in zip(ids, kinds):
                got = self.batch_torch(rows, int(kind), ssl=ssl) if torch else self.batch(rows, int(kind), ssl=ssl)
                yield (*got, rows, int(kind))
            epoch += 1

    # ---- weights (include/m0_batch_weighted.h) ----
    def set_weights(self, ids, values) -> None:
        """One weight per id.  numpy arrays (or sequences): checked -- ValueError, with nothing changed, for an id that is not
        resident or occurs twice and for a value that is not finite in [0, 65536] -- and in place when the call returns.  torch
        CUDA tensors (i64 and f32 on the store's device): enqueued on torch's current stream without a wait; values are
        sanitised and ids outside the window skipped on the device, both counted in weights_info(); of two values for one id
        one is stored."""
        if hasattr(ids, "data_ptr") or hasattr(values, "data_ptr"):
            import torch
            if self.device == ROWSTORE_HOST:
                raise ValueError("a host store takes weights from host memory")
            dev = torch.device("cuda", self.device)
            for t, dtype in ((ids, torch.int64), (values, torch.float32)):
                if not hasattr(t, "data_ptr") or t.dtype != dtype or t.device != dev or not t.is_contiguous() or t.dim() != 1:
                    raise ValueError(f"ids and values must be contiguous 1-d i64 and f32 tensors on {dev}")
            if len(ids) != len(values):
                raise ValueError("one value per id")
            stream = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(self._L.m0_rowstore_set_weights(self._h, C.c_void_p(ids.data_ptr()), C.c_void_p(values.data_ptr()), len(ids), 1,
                                                       C.c_void_p(stream)), "m0_rowstore_set_weights")
            return
        ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        values = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
        if len(ids) != len(values):
            raise ValueError("one value per id")
        _lib.check(self._L.m0_rowstore_set_weights(self._h, _lib.ptr(ids), _lib.ptr(values), len(ids), 0, None), "m0_rowstore_set_weights")

    def fill_weights(self, ids_range: range, value: float) -> None:
        """Every row of a range of consecutive ids (as append returns it) gets `value`: how new rows get the highest priority."""
        r = range(ids_range.start, ids_range.stop) if isinstance(ids_range, range) and ids_range.step == 1 else None
        if r is None:
            raise ValueError("ids_range must be a range of consecutive ids")
        _lib.check(self._L.m0_rowstore_fill_weights(self._h, r.start, len(r), float(value)), "m0_rowstore_fill_weights")

    def scale_weights(self, factor: float) -> None:
        """w = min(65536, w * factor) for every resident row: one call per append is an exponential decay by age."""
        _lib.check(self._L.m0_rowstore_scale_weights(self._h, float(factor)), "m0_rowstore_scale_weights")

    def weights(self, ids) -> np.ndarray:
        """f32 [n]: the weights of these resident ids, after everything enqueued on the device has finished."""
        ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        out = np.empty(len(ids), np.float32)
        _lib.check(self._L.m0_rowstore_get_weights(self._h, _lib.ptr(ids), len(ids), _lib.ptr(out)), "m0_rowstore_get_weights")
        return out

    def weights_info(self) -> dict:
        """total_ticks (a weight of 1 is 2^24 ticks), rows_with_ticks, and two counts over the life of the store: the values
        sanitised or ids skipped by set_weights from tensors, and the draws made from a total of 0 (uniform instead)."""
        out = np.zeros(len(WEIGHTS_INFO), np.int64)
        _lib.check(self._L.m0_rowstore_weights_info(self._h, _lib.ptr(out)), "m0_rowstore_weights_info")
        return dict(zip(WEIGHTS_INFO, (int(x) for x in out)))

    def reweigh(self, backend, rule, batch_size: int = 1024, **score_options) -> dict:
        """Every resident row scored by `backend` (M0Backend.score_resident, in id order, batch_size rows a call) and given the
        rule's weight of its columns on the device.  Returns the means of the rule's inputs over the scored rows: policy_loss,
        entropy, value_loss, and rows."""
        ids = self.resident_ids()
        sums = np.zeros(3, np.float64)
        for at in range(0, len(ids), int(batch_size)):
            rows = backend.score_resident(self, ids[at:at + int(batch_size)], rule=rule, **score_options)
            sums += rows[:, :3].sum(axis=0, dtype=np.float64)
        mean = sums / max(len(ids), 1)
        return {"policy_loss": float(mean[0]), "entropy": float(mean[1]), "value_loss": float(mean[2]), "rows": len(ids)}

    def _draw_outputs(self, B: int, torch: bool):
        """(ids, prob, their pointers, outputs_on_device, stream) of a draw"""
        if not torch:
            ids, prob = np.empty(B, np.int64), np.empty(B, np.float32)
            return ids, prob, [_lib.ptr(ids), _lib.ptr(prob)], 0, None
        import torch as th
        if self.device == ROWSTORE_HOST:
            raise ValueError("a host store has no device tensors")
        dev = th.device("cuda", self.device)
        ids, prob = th.empty(B, dtype=th.int64, device=dev), th.empty(B, dtype=th.float32, device=dev)
        return ids, prob, [C.c_void_p(ids.data_ptr()), C.c_void_p(prob.data_ptr())], 1, C.c_void_p(th.cuda.current_stream(dev).cuda_stream)

    def sample(self, B: int, seed: int, draw: int, stratified: bool = False, torch: bool = False):
        """(ids i64 [B], prob f32 [B]): B rows drawn in proportion to their weights, a function of (seed, draw, B, stratified) and
        the weights; prob is each row's share of the total weight.  stratified cuts the total into B equal spans and draws one
        row from each: ids ascend.  numpy arrays, or with torch=True tensors filled on torch's current stream without a wait."""
        B = int(B)
        ids, prob, ptrs, on_device, stream = self._draw_outputs(max(B, 0), torch)
        _lib.check(self._L.m0_rowstore_sample(self._h, B, int(seed) & U64, int(draw) & U64, int(bool(stratified)), *ptrs, on_device, stream),
                   "m0_rowstore_sample")
        return ids, prob

    def sampled_batch(self, B: int, seed: int, draw: int, kinds=None, stratified: bool = False, ssl: bool = False, torch: bool = False,
                      out=None):
        """sample() and the batch of the drawn rows behind it on the device: what batch() -- with torch=True, batch_torch() --
        returns for (ids, kinds), then ids and prob.  The draw hands the rows to the gather on the device; with torch=True nothing
        waits for either.  out: the batch tensors of an earlier torch=True call, to be written again."""
        B = int(B)
        n = max(B, 0)
        _, kinds = self._ids_kinds(np.zeros(n, np.int64), kinds)
        if torch:
            import torch as th
            dev = th.device("cuda", self.device) if self.device != ROWSTORE_HOST else None
        ids, prob, draw_ptrs, on_device, stream = self._draw_outputs(n, torch)
        if torch:
            want = [((n, PLANES, 8, 8), th.float32), ((n, POLICY_SIZE), th.float32), ((n,), th.float32)]
            if self.with_mask:
                want.append(((n, POLICY_SIZE), th.uint8))
            if ssl:
                want += [((n, BATCH_SSL_CH, 8, 8), th.float32), ((n,), th.int32)]
            if out is None:
                out = tuple(th.empty(shape, dtype=dtype, device=dev) for shape, dtype in want)
            out = tuple(out)
            if len(out) != len(want) or any(tuple(t.shape) != shape or t.dtype != dtype or t.device != dev or not t.is_contiguous()
                                            for t, (shape, dtype) in zip(out, want)):
                raise ValueError(f"out must be contiguous tensors on {dev} of {want}")
            ptrs = [C.c_void_p(t.data_ptr()) for t in out]
        else:
            if out is not None:
                raise ValueError("out is for torch=True")
            out = [np.empty((n, PLANES, 8, 8), np.float32), np.empty((n, POLICY_SIZE), np.float32), np.empty(n, np.float32)]
            if self.with_mask:
                out.append(np.empty((n, POLICY_SIZE), np.uint8))
            if ssl:
                out += [np.empty((n, BATCH_SSL_CH, 8, 8), np.float32), np.empty(n, np.int32)]
            out = tuple(out)
            ptrs = [_lib.ptr(a) for a in out]
        if not self.with_mask:
            ptrs.insert(3, None)
        if not ssl:
            ptrs += [None, None]
        _lib.check(self._L.m0_rowstore_batch_sampled(self._h, B, int(seed) & U64, int(draw) & U64, int(bool(stratified)), _lib.ptr(kinds), *ptrs,
                                                     *draw_ptrs, on_device, stream), "m0_rowstore_batch_sampled")
        return (*out, ids, prob)


def weight_rule(policy: float = 1.0, kl: float = 0.0, value: float = 0.0, floor: float = 0.0, cap: float = float(WEIGHT_MAX)):
    """How a row's score columns become its weight (m0_weight_rule): w = min(cap, max(0, floor + policy * policy_loss +
    kl * (policy_loss - entropy) + value * value_loss)), built with three fused multiply-adds in float32 in that order.  No
    exponent: a PER alpha is the caller's."""
    return WeightRule(float(policy), float(kl), float(value), float(floor), float(cap))


def weight_from_score(rows, rule) -> np.ndarray:
    """f32 [B]: the rule's weights of score rows f32 [B, 8] (M0Backend.score and its kin), the function the device runs
    (m0_weight_from_score)."""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    if rows.ndim != 2 or rows.shape[1] != SCORE_COLS:
        raise ValueError(f"rows must be [B, {SCORE_COLS}]")
    out = np.empty(len(rows), np.float32)
    _lib.check(_lib.lib().m0_weight_from_score(_lib.ptr(rows), len(rows), C.byref(rule), _lib.ptr(out)), "m0_weight_from_score")
    return out


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
