"""Packed training rows (include/m0_rowpack.h): a stored row -- s f32 [19,8,8], pi f32 [4672], legal_mask u8 [4672], z -- is
28 228 bytes dense and a few hundred packed: twelve bitboards, a few scalars, the non-zero entries of pi, and the mask only where
it is not the position's legal moves.  Nothing is lossy: what the packed form cannot give back bit for bit stays dense ("raw").

    packed = pack_rows(s, pi, z, legal_mask)            # the device when there is one, else the same code on the CPU
    s, pi, z, legal_mask = unpack_rows(packed)
    save_packed(path, packed, extra)                    # an .npz with a rowpack_version key
    load_shard(path)                                    # the dense dict of either kind of file

    python -m matrix0_amd.rowpack pack|unpack|info SRC [DST]

pack and unpack take one shard, or a store directory (its *.npz anywhere below, the `shards` table of its data_metadata.db kept
in step through ShardIndex).  Every other key of a shard (meta_*, ssl_*, traces) passes through unchanged."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import shutil
import sys
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, Optional

import numpy as np

from . import _lib
from ._abi import POLICY_SIZE, ROWPACK_MASK_KINDS, ROWPACK_ROW_KINDS, ROWPACK_VERSION, RowpackArrays, RowpackPos
from .data_writer import ShardIndex, write_npz

PLANES = 19
POS_BYTES = C.sizeof(RowpackPos)
DENSE_ROW_BYTES = PLANES * 64 * 4 + POLICY_SIZE * 4 + POLICY_SIZE + 4
# m0_rowpack_pos as numpy sees it (little endian, no padding: 104 bytes)
POS_DTYPE = np.dtype([("men", "<u8", (12,)), ("turn", "u1"), ("castling", "u1"), ("ep", "u1"), ("halfmove", "u1"),
                      ("fullmove", "u1"), ("row_kind", "u1"), ("mask_kind", "u1"), ("reserved", "u1")])
assert POS_DTYPE.itemsize == POS_BYTES == 104
ARRAY_KEYS = ("pos", "z", "pi_off", "pi_idx", "pi_val", "mask_off", "mask_idx", "raw_planes", "raw_pi", "raw_mask")
DENSE_KEYS = ("s", "pi", "z", "legal_mask")


@dataclass
class PackedRows:
    """The arrays of m0_rowpack_arrays.  pos u8 [n,104] (view it with POS_DTYPE), z f32 [n], pi_off i64 [n+1], pi_idx u16,
    pi_val f32, mask_off i64 [n+1], mask_idx u16, raw_planes f32 [r,19,8,8], raw_pi f32 [r,4672], raw_mask u8 [r,4672] or None
    (rows without masks)."""
    pos: np.ndarray
    z: np.ndarray
    pi_off: np.ndarray
    pi_idx: np.ndarray
    pi_val: np.ndarray
    mask_off: np.ndarray
    mask_idx: np.ndarray
    raw_planes: np.ndarray
    raw_pi: np.ndarray
    raw_mask: Optional[np.ndarray]

    @property
    def n(self) -> int:
        return int(self.pos.shape[0])

    @property
    def nbytes(self) -> int:
        return int(sum(getattr(self, k).nbytes for k in ARRAY_KEYS if getattr(self, k) is not None))

    @property
    def fields(self) -> np.ndarray:
        return self.pos.view(POS_DTYPE).reshape(-1)

    @property
    def has_mask(self) -> bool:
        return self.n > 0 and int(self.fields["mask_kind"][0]) != ROWPACK_MASK_KINDS["none"]

    def kinds(self) -> Dict[str, Dict[str, int]]:
        f = self.fields
        return {"rows": {k: int((f["row_kind"] == v).sum()) for k, v in ROWPACK_ROW_KINDS.items()},
                "masks": {k: int((f["mask_kind"] == v).sum()) for k, v in ROWPACK_MASK_KINDS.items()}}

    def validate(self) -> None:
        """ValueError unless every array has the type, shape and length that m0_rowpack_arrays says (a truncated or wrongly
        typed key of a packed file would otherwise be read past its end)."""
        n = self.pos.shape[0] if isinstance(self.pos, np.ndarray) and self.pos.ndim == 2 else -1
        raw = self.raw_planes.shape[0] if isinstance(self.raw_planes, np.ndarray) and self.raw_planes.ndim >= 1 else -1
        want = {"pos": (np.uint8, (n, POS_BYTES)), "z": (np.float32, (n,)), "pi_off": (np.int64, (n + 1,)),
                "pi_idx": (np.uint16, (-1,)), "pi_val": (np.float32, (-1,)), "mask_off": (np.int64, (n + 1,)),
                "mask_idx": (np.uint16, (-1,)), "raw_planes": (np.float32, (raw, PLANES, 8, 8)),
                "raw_pi": (np.float32, (raw, POLICY_SIZE)), "raw_mask": (np.uint8, (raw, POLICY_SIZE))}
        if n <= 0:
            raise ValueError("packed rows: pos must be u8 [n,104] with n > 0")
        for k, (dtype, shape) in want.items():
            v = getattr(self, k)
            if v is None and k == "raw_mask":
                continue
            if not isinstance(v, np.ndarray) or v.dtype != dtype or not v.flags.c_contiguous or v.ndim != len(shape) or \
                    any(w >= 0 and g != w for g, w in zip(v.shape, shape)):
                raise ValueError(f"packed rows: {k} must be {np.dtype(dtype).name} {list(shape)} (-1: any length), got "
                                 f"{getattr(v, 'dtype', type(v).__name__)} {list(getattr(v, 'shape', ()))}")
        if len(self.pi_idx) != len(self.pi_val):
            raise ValueError("packed rows: pi_idx and pi_val differ in length")

    def c_arrays(self) -> RowpackArrays:
        """The struct the library takes; the arrays must stay alive while it is used.  The library sees pointers and counts: what
        it cannot check -- types, shapes, contiguity and the lengths that go with n -- is checked here (ValueError)."""
        self.validate()
        a = RowpackArrays()
        a.n, a.pi_n, a.mask_n, a.raw_n = self.n, len(self.pi_idx), len(self.mask_idx), len(self.raw_planes)
        for k in ARRAY_KEYS:
            v = getattr(self, k)
            setattr(a, k, None if v is None or v.size == 0 else v.ctypes.data)
        return a

    def rows(self, lo: int, hi: int) -> "PackedRows":
        """Rows lo .. hi - 1 as packed rows of their own (offsets rebased)."""
        f = self.fields
        raw = np.concatenate([[0], np.cumsum(f["row_kind"] == ROWPACK_ROW_KINDS["raw"])])
        p0, p1, m0, m1, r0, r1 = (int(self.pi_off[lo]), int(self.pi_off[hi]), int(self.mask_off[lo]), int(self.mask_off[hi]),
                                  int(raw[lo]), int(raw[hi]))
        return PackedRows(np.ascontiguousarray(self.pos[lo:hi]), np.ascontiguousarray(self.z[lo:hi]), self.pi_off[lo:hi + 1] - p0,
                          np.ascontiguousarray(self.pi_idx[p0:p1]), np.ascontiguousarray(self.pi_val[p0:p1]),
                          self.mask_off[lo:hi + 1] - m0, np.ascontiguousarray(self.mask_idx[m0:m1]),
                          np.ascontiguousarray(self.raw_planes[r0:r1]), np.ascontiguousarray(self.raw_pi[r0:r1]),
                          None if self.raw_mask is None else np.ascontiguousarray(self.raw_mask[r0:r1]))


def _use_device(device) -> Optional[int]:
    """device: a HIP device, "host" for the CPU, None for device 0 when there is one and the CPU otherwise"""
    if device == "host":
        return None
    if device is not None:
        return int(device)
    return 0 if _lib.device_count() > 0 else None


def mask_mode_of(packed: PackedRows, mask_mode: Optional[str] = None) -> str:
    """backend.resolve_mask_mode read off packed rows: "legal" with masks; without, "none" when every row has exactly one
    positive pi entry and "target" otherwise."""
    if mask_mode is not None:
        return mask_mode
    if packed.has_mask:
        return "legal"
    positive = np.concatenate([[0], np.cumsum(packed.pi_val > 0)])[packed.pi_off]
    count = (positive[1:] - positive[:-1]).astype(np.int64)
    count[packed.fields["row_kind"] == ROWPACK_ROW_KINDS["raw"]] = (packed.raw_pi > 0).sum(axis=1)
    return "none" if bool((count == 1).all()) else "target"


def _dense(s, pi, z, legal_mask):
    s = np.ascontiguousarray(s, dtype=np.float32)
    n = s.shape[0]
    if n <= 0 or s.size != n * PLANES * 64:
        raise ValueError("s must be f32 [n,19,8,8] with n > 0")
    pi = None if pi is None else np.ascontiguousarray(pi, dtype=np.float32)
    z = np.ascontiguousarray(z, dtype=np.float32)
    if (pi is not None and pi.shape != (n, POLICY_SIZE)) or z.size != n:
        raise ValueError("pi must be f32 [n,4672] and z f32 [n]")
    if legal_mask is not None:
        legal_mask = np.ascontiguousarray(legal_mask)
        if legal_mask.dtype == np.bool_:
            legal_mask = legal_mask.view(np.uint8)
        if legal_mask.dtype != np.uint8 or legal_mask.size != n * POLICY_SIZE:
            raise ValueError("legal_mask must be u8 [n,4672]")
    return s, pi, z, legal_mask


def pack_rows(s, pi, z, legal_mask=None, device=None) -> PackedRows:
    """Dense rows -> PackedRows; on the device when one is given or available, else on the CPU: the same arrays either way.
    pi None: rows without a policy, which pack as rows of zeros do (pack_rows_onehot)."""
    s, pi, z, legal_mask = _dense(s, pi, z, legal_mask)
    n = s.shape[0]
    L = _lib.lib()
    dev = _use_device(device)
    sizes = np.zeros(3, np.int64)
    # a first guess that nearly always holds (real rows: 1 to 45 entries, no LIST mask, no raw row); the sizes come back either way
    caps = [n * 48 + 4096, 4096, 4]
    for attempt in range(2):
        out = PackedRows(np.zeros((n, POS_BYTES), np.uint8), np.empty(n, np.float32), np.empty(n + 1, np.int64),
                         np.empty(caps[0], np.uint16), np.empty(caps[0], np.float32), np.empty(n + 1, np.int64),
                         np.empty(caps[1], np.uint16), np.empty((caps[2], PLANES, 8, 8), np.float32),
                         np.empty((caps[2], POLICY_SIZE), np.float32),
                         None if legal_mask is None else np.empty((caps[2], POLICY_SIZE), np.uint8))
        a = out.c_arrays()
        args = (_lib.ptr(s), _lib.ptr(pi), _lib.ptr(z), _lib.ptr(legal_mask), n, C.byref(a), _lib.ptr(sizes))
        rc = L.m0_rowpack_pack_host(*args) if dev is None else L.m0_rowpack_pack(dev, *args)
        if rc == _lib.M0_OK:
            break
        if attempt == 1 or rc != _lib.M0_ERR_INVALID or all(int(sizes[k]) <= caps[k] for k in range(3)):
            _lib.check(rc, "m0_rowpack_pack")
        caps = [int(x) for x in sizes]
    npi, nmk, raw = (int(x) for x in sizes)
    out.pi_idx, out.pi_val, out.mask_idx = out.pi_idx[:npi].copy(), out.pi_val[:npi].copy(), out.mask_idx[:nmk].copy()
    out.raw_planes, out.raw_pi = out.raw_planes[:raw].copy(), out.raw_pi[:raw].copy()
    if out.raw_mask is not None:
        out.raw_mask = out.raw_mask[:raw].copy()
    return out


def pack_rows_onehot(s, move_idx, z, legal_mask=None, device=None) -> PackedRows:
    """pack_rows of rows whose pi is 1.0 at column move_idx[i] and 0 elsewhere (imported games), without that pi ever being
    built: the rows are packed without a policy, and the one entry of each is written here -- the arrays are those that
    pack_rows gives for the dense one-hot rows."""
    idx = np.asarray(move_idx).astype(np.int64).reshape(-1)
    out = pack_rows(s, None, z, legal_mask, device)
    if len(idx) != out.n or (idx < 0).any() or (idx >= POLICY_SIZE).any():
        raise ValueError("move_idx must hold one column below 4672 per row")
    packed = out.fields["row_kind"] == ROWPACK_ROW_KINDS["packed"]
    out.pi_off = np.concatenate([[0], np.cumsum(packed)]).astype(np.int64)
    out.pi_idx = idx[packed].astype(np.uint16)
    out.pi_val = np.ones(int(packed.sum()), np.float32)
    out.raw_pi[np.arange(len(out.raw_pi)), idx[~packed]] = 1.0
    return out


def unpack_rows(packed: PackedRows, device=None):
    """PackedRows -> (s f32 [n,19,8,8], pi f32 [n,4672], z f32 [n], legal_mask u8 [n,4672] or None), bit for bit what was packed."""
    packed.validate()
    n = packed.n
    s, pi, z = np.empty((n, PLANES, 8, 8), np.float32), np.empty((n, POLICY_SIZE), np.float32), np.empty(n, np.float32)
    mask = np.empty((n, POLICY_SIZE), np.uint8) if packed.has_mask else None
    a = packed.c_arrays()
    L = _lib.lib()
    dev = _use_device(device)
    args = (C.byref(a), _lib.ptr(s), _lib.ptr(pi), _lib.ptr(z), _lib.ptr(mask))
    _lib.check(L.m0_rowpack_unpack_host(*args) if dev is None else L.m0_rowpack_unpack(dev, *args), "m0_rowpack_unpack")
    return s, pi, z, mask


# ---- files ----
def is_packed(d) -> bool:
    return "rowpack_version" in (d.files if hasattr(d, "files") else d)


def packed_from_dict(d) -> PackedRows:
    version = int(np.asarray(d["rowpack_version"]).reshape(-1)[0])
    if version != ROWPACK_VERSION:
        raise ValueError(f"rowpack_version {version}: this build reads version {ROWPACK_VERSION}")
    get = lambda k: np.ascontiguousarray(d["rowpack_" + k])
    has_raw_mask = int(np.asarray(d["rowpack_has_mask"]).reshape(-1)[0]) != 0
    return PackedRows(get("pos"), get("z"), get("pi_off"), get("pi_idx"), get("pi_val"), get("mask_off"), get("mask_idx"),
                      get("raw_planes"), get("raw_pi"), get("raw_mask") if has_raw_mask else None)


def packed_to_dict(packed: PackedRows, extra: Optional[Dict[str, np.ndarray]] = None, shapes=None) -> Dict[str, np.ndarray]:
    """The keys of a packed shard.  shapes: {"z": ..., "legal_mask": ..., "legal_mask_dtype": ...} of the dense arrays where they
    were not [n] / u8 [n,4672] (the reference also writes z [n,1] and masks [n,73,8,8] or bool), so that unpacking restores them."""
    out = {"rowpack_version": np.array([ROWPACK_VERSION], np.int32),
           "rowpack_has_mask": np.array([1 if packed.raw_mask is not None else 0], np.int32)}
    for k in ARRAY_KEYS:
        v = getattr(packed, k)
        out["rowpack_" + k] = v if v is not None else np.zeros((0, POLICY_SIZE), np.uint8)
    if shapes:
        out["rowpack_shapes"] = np.array(json.dumps(shapes))
    for k, v in (extra or {}).items():
        if k in DENSE_KEYS or k.startswith("rowpack_"):
            raise ValueError(f"extra key {k} collides with the rows' own")
        out[k] = v
    return out


def save_packed(path, packed: PackedRows, extra: Optional[Dict[str, np.ndarray]] = None, shapes=None) -> None:
    write_npz(path, packed_to_dict(packed, extra, shapes))


def read_shard(path, keys=None):
    """(PackedRows or None, dict): a packed file's rows and its other keys; a dense file's dict.  Which kind a file is comes from
    the names in it, before any array is read.  keys: read only these of the keys that are not the packed rows' own (None: all),
    so a caller that wants s, pi, z and legal_mask inflates nothing else, and keys=() reads a packed file's rows and nothing of a
    dense file."""
    with np.load(path, allow_pickle=False) as d:
        packed = "rowpack_version" in d.files
        own = [k for k in d.files if packed and k.startswith("rowpack_")]
        data = {k: d[k] for k in d.files if k in own or keys is None or k in keys}
    if not packed:
        return None, data
    return packed_from_dict(data), {k: v for k, v in data.items() if not k.startswith("rowpack_") or k == "rowpack_shapes"}


def load_shard(path, device=None, keys=None) -> Dict[str, np.ndarray]:
    """The dense dict of a dense or a packed shard: s, pi, z, legal_mask (where the rows had one) and every other key, or only
    those of `keys` (the others are not read)."""
    packed, rest = read_shard(path, keys)
    if packed is None:
        return rest
    s, pi, z, mask = unpack_rows(packed, device)
    shapes = json.loads(str(rest.pop("rowpack_shapes"))) if "rowpack_shapes" in rest else {}
    out = {"s": s, "pi": pi, "z": z.reshape(shapes.get("z", z.shape))}
    if mask is not None:
        if shapes.get("legal_mask_dtype") == "bool":
            mask = mask.view(np.bool_)
        out["legal_mask"] = mask.reshape(shapes.get("legal_mask", mask.shape))
    if keys is not None:
        out = {k: v for k, v in out.items() if k in keys}
    out.update(rest)
    return out


def pack_dict(data: Dict[str, np.ndarray], device=None) -> Dict[str, np.ndarray]:
    """A dense shard's dict as a packed shard's."""
    s, pi, z = np.asarray(data["s"]), np.asarray(data["pi"]), np.asarray(data["z"])
    lm = np.asarray(data["legal_mask"]) if "legal_mask" in data else None
    if s.dtype != np.float32 or pi.dtype != np.float32 or z.dtype != np.float32 or (lm is not None and lm.dtype not in (np.uint8, np.bool_)):
        raise ValueError("a shard packs from float32 s, pi, z and a uint8 or bool legal_mask")
    shapes = {}
    if z.shape != (s.shape[0],):
        shapes["z"] = list(z.shape)
    if lm is not None and lm.shape != (s.shape[0], POLICY_SIZE):
        shapes["legal_mask"] = list(lm.shape)
    if lm is not None and lm.dtype == np.bool_:
        shapes["legal_mask_dtype"] = "bool"
    packed = pack_rows(s, pi, z.reshape(-1), None if lm is None else lm.reshape(s.shape[0], -1), device)
    return packed_to_dict(packed, {k: v for k, v in data.items() if k not in DENSE_KEYS}, shapes)


# ---- command line ----
def _shards(src: Path):
    return [src] if src.is_file() else sorted(p for p in src.rglob("*.npz") if p.is_file())


def _convert(src: Path, dst: Path, to_packed: bool, device=None) -> Dict[str, int]:
    """Every shard of src (a file or a store directory) into dst in the other form; the `shards` rows of a store follow.  A file
    that is already in that form, or holds no rows (no s, pi and z: the readers skip it too), is copied as it is.  Returns the
    counts of files and of files without rows."""
    files = _shards(src)
    sources, without_rows = {}, 0
    if src.is_dir():
        sources = {str(Path(p).resolve()): s for p, _, s, corrupted in ShardIndex(src, create=False).rows() if not corrupted}
    if src.is_dir():
        dst.mkdir(parents=True, exist_ok=True)
    index = ShardIndex(dst) if sources else None
    for f in files:
        out = dst / f.relative_to(src) if src.is_dir() else dst
        out.parent.mkdir(parents=True, exist_ok=True)
        with np.load(f, allow_pickle=False) as d:
            names = set(d.files)
        src_key = str(f.resolve())
        is_rows = "rowpack_version" in names or {"s", "pi", "z"} <= names
        if not is_rows or ("rowpack_version" in names) == to_packed:
            # no rows in it (the readers skip such a file too), or already in the form asked for: the file as it is
            shutil.copyfile(f, out)
            without_rows += 0 if is_rows else 1
            rows = 0
            if is_rows:
                with np.load(f, allow_pickle=False) as d:
                    rows = d["rowpack_pos" if "rowpack_version" in names else "s"].shape[0]
        else:
            payload = pack_dict(read_shard(f)[1], device) if to_packed else load_shard(f, device)
            write_npz(out, payload)
            rows = payload["rowpack_pos"].shape[0] if to_packed else np.asarray(payload["s"]).shape[0]
        if index is not None and src_key in sources:
            index.add(out, int(rows), sources[src_key] or "selfplay")
    return {"shards": len(files), "without_rows": without_rows}


def info(src: Path) -> Dict:
    """Counts of row and mask kinds and bytes per row over the shards of src."""
    out = {"shards": 0, "dense_shards": 0, "rows": 0, "rows_by_kind": {k: 0 for k in ROWPACK_ROW_KINDS},
           "masks_by_kind": {k: 0 for k in ROWPACK_MASK_KINDS}, "packed_bytes": 0, "file_bytes": 0}
    for f in _shards(src):
        packed, data = read_shard(f, DENSE_KEYS)
        if packed is None and not {"s", "pi", "z"} <= set(data):
            continue                                        # no rows in it
        out["shards"] += 1
        out["file_bytes"] += os.path.getsize(f)
        if packed is None:
            out["dense_shards"] += 1
            packed = pack_rows(data["s"], data["pi"], np.asarray(data["z"]).reshape(-1),
                               np.asarray(data["legal_mask"]).reshape(len(data["s"]), -1) if "legal_mask" in data else None)
        kinds = packed.kinds()
        out["rows"] += packed.n
        out["packed_bytes"] += packed.nbytes
        for k, v in kinds["rows"].items():
            out["rows_by_kind"][k] += v
        for k, v in kinds["masks"].items():
            out["masks_by_kind"][k] += v
    rows = max(out["rows"], 1)
    out["packed_bytes_per_row"] = out["packed_bytes"] / rows
    out["file_bytes_per_row"] = out["file_bytes"] / rows
    out["dense_bytes_per_row"] = DENSE_ROW_BYTES
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m matrix0_amd.rowpack", description=__doc__.split("\n\n")[0])
    ap.add_argument("command", choices=("pack", "unpack", "info"))
    ap.add_argument("src")
    ap.add_argument("dst", nargs="?")
    ap.add_argument("--device", default=None, help="a HIP device or `host` (default: device 0 when there is one, else the CPU)")
    a = ap.parse_args(argv)
    src = Path(a.src)
    if not src.exists():
        ap.error(f"{src} does not exist")
    if a.command == "info":
        print(json.dumps(info(src)))
        return 0
    if not a.dst:
        ap.error(f"{a.command} needs a destination")
    if src.is_dir() and Path(a.dst).resolve() == src.resolve():
        ap.error("the destination must be another directory")
    print(json.dumps(dict(_convert(src, Path(a.dst), a.command == "pack", a.device), command=a.command)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
