"""Rows shared by tests/test_rowpack.py (CPU) and tests/test_rowpack_gpu.py: the golden worker rows, and sets built from them in
which every row kind, mask kind and pi entry-count edge of include/m0_rowpack.h occurs."""
import functools
import glob
import os

import numpy as np

from tests import planes_cases as pc

HERE = os.path.dirname(os.path.abspath(__file__))
COLS = 4672
PACKED, RAW = 0, 1
MASK_NONE, MASK_LEGAL, MASK_LIST = 0, 1, 2
# bit patterns that are entries although they compare equal to 0.0 or to nothing: -0.0, the smallest denormal, two NaN payloads
ODD_BITS = np.array([0x80000000, 0x00000001, 0x7FC00001, 0xFFA5A5A5], np.uint32)
ENTRY_COUNTS = (0, 1, 63, 64, 65, 218, 4672)
EDGES = 16


@functools.lru_cache(maxsize=None)
def worker_rows():
    """(s f32 [375,19,8,8], pi f32 [375,4672], z f32 [375], legal_mask u8 [375,4672]) of the nine golden self-play games"""
    parts = [np.load(f) for f in sorted(glob.glob(os.path.join(HERE, "golden", "ref_worker_*.npz")))]
    s = np.concatenate([d["s"] for d in parts]).astype(np.float32)
    pi = np.concatenate([d["pi"] for d in parts]).astype(np.float32)
    z = np.concatenate([d["z"].reshape(-1) for d in parts]).astype(np.float32)
    mask = np.concatenate([d["legal_mask"].reshape(len(d["s"]), -1) for d in parts]).astype(np.uint8)
    assert len(s) == 375
    for a in (s, pi, z, mask):
        a.setflags(write=False)
    return s, pi, z, mask


def seeded_pi(rng, count, columns=None):
    """A pi row with `count` entries at seeded columns (or exactly at `columns`), values in (0, 1]"""
    row = np.zeros(COLS, np.float32)
    cols = np.asarray(columns) if columns is not None else rng.choice(COLS, size=count, replace=False)
    row[cols] = (rng.random(len(cols), dtype=np.float32) * 0.999 + 0.001).astype(np.float32)
    return row


def edge_rows(B, seed, with_mask=True):
    """B rows cycling through EDGES kinds of row (row i is kind (i + seed) % EDGES), built on the worker rows: what each kind
    must pack to is in expected_kinds.  Returns (s, pi, z, mask or None, kinds i32 [B])."""
    ws, wpi, wz, wm = worker_rows()
    rng = np.random.default_rng(seed)
    src = rng.integers(0, len(ws), size=B)
    s, pi, z, mask = ws[src].copy(), wpi[src].copy(), wz[src].copy(), wm[src].copy()
    kinds = (np.arange(B) + seed) % EDGES
    for i, k in enumerate(kinds):
        legal, illegal = np.flatnonzero(mask[i]), np.flatnonzero(mask[i] == 0)
        if k == 1:
            mask[i, legal[rng.integers(len(legal))]] = 0              # one legal bit cleared
        elif k == 2:
            mask[i, illegal[rng.integers(len(illegal))]] = 1          # one illegal bit set
        elif k == 3:
            mask[i, legal[0]] = 2                                     # a byte that is neither 0 nor 1
        elif k == 4:
            s[i, 3, 4, 4] = 0.5                                       # no position: a piece-plane value
        elif 5 <= k <= 11:
            pi[i] = seeded_pi(rng, ENTRY_COUNTS[k - 5])
        elif k == 12:
            pi[i] = seeded_pi(rng, 4, [0, 63, 64, 4671])
        elif k == 13:
            pi[i] = seeded_pi(rng, 16, np.arange(COLS - 16, COLS))    # the last 16-byte piece group only
        elif k == 14:
            pi[i] = 0.0
            pi[i].view(np.uint32)[rng.choice(COLS, size=4, replace=False)] = ODD_BITS
        elif k == 15:
            s[i, 17, 7, 7] = 0.25                                     # no position: a counter plane that varies
    return s, pi, z, (mask if with_mask else None), kinds.astype(np.int32)


def expected_kinds(kinds, with_mask=True):
    """(row kinds, mask kinds) that edge_rows' rows must pack to"""
    kinds = np.asarray(kinds)
    raw = np.isin(kinds, (4, 15)) | (with_mask & (kinds == 3))
    rows = np.where(raw, RAW, PACKED)
    if not with_mask:
        return rows, np.full(len(kinds), MASK_NONE)
    return rows, np.where(raw | np.isin(kinds, (1, 2)), MASK_LIST, MASK_LEGAL)


def ep_rows():
    """The 13 hand-written en-passant positions as rows: (s, pi, z, mask, ep squares or None)"""
    enc = [pc.encode(fen) for fen, _ in pc.EP_FENS]
    s, mask = np.stack([e[0] for e in enc]).astype(np.float32), np.stack([e[1] for e in enc]).astype(np.uint8)
    pi = (mask / mask.sum(axis=1, keepdims=True)).astype(np.float32)
    return s, pi, np.linspace(-1, 1, len(s)).astype(np.float32), mask, [ep for _, ep in pc.EP_FENS]


def same_bits(a, b):
    """Bitwise equality of two arrays (None equals None): uint32 patterns of floats, bytes of everything else"""
    if a is None or b is None:
        return a is None and b is None
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


def same_packed(a, b):
    """Two PackedRows array by array; the first key that differs, or None"""
    for k in ("pos", "z", "pi_off", "pi_idx", "pi_val", "mask_off", "mask_idx", "raw_planes", "raw_pi", "raw_mask"):
        if not same_bits(getattr(a, k), getattr(b, k)):
            return k
    return None
