"""Device-side azchess/encoding.py (reference file:line in each docstring), FEN-addressed.

The reference takes python-chess Board objects; a caller that keeps python-chess passes
``board.fen()`` (and ``move.uci()``).  Everything is computed by the HIP kernels behind
m0_encode_fens (one wave per position); there is no CPU implementation in this package."""
from __future__ import annotations

import ctypes as C
from typing import List, Sequence, Tuple

import numpy as np

from . import _lib
from ._abi import (AUGMENT_KINDS, DECODE_MASK_MISMATCH, DECODE_OK, DECODE_STATUS, EP_FROM_MASK, FULLMOVE_SATURATED,  # noqa: F401
                   HALFMOVE_SATURATED, NO_MASK)
from ._lib import ptr
from .engine import move_to_uci

POLICY_SHAPE = (8, 8, 73)
LEGACY_POLICY_SIZE = 4672


def encode_fens(fens: Sequence[str], device_index: int = 0, want_moves: bool = True):
    """Batched: planes f32 [n,19,8,8], mask bool [n,4672], per-position (ucis, indices) in
    legal_moves order."""
    n = len(fens)
    planes = np.empty((n, 19, 8, 8), np.float32)
    mask = np.empty((n, 4672), np.uint8)
    nl = np.empty((n,), np.int32)
    mv = np.empty((n, 256), np.uint16)
    idx = np.empty((n, 256), np.int32)
    _lib.check(_lib.lib().m0_encode_fens(int(device_index), _lib.cstrings(fens), n, ptr(planes), ptr(mask), ptr(nl), ptr(mv),
                                         ptr(idx)), "m0_encode_fens")
    moves = None
    if want_moves:
        moves = [([move_to_uci(int(m)) for m in mv[i, : nl[i]]], idx[i, : nl[i]].tolist()) for i in range(n)]
    return planes, mask.astype(bool), moves


def decode_planes(planes, mask=None, device_index: int = 0) -> dict:
    """The way back from stored rows: planes f32 [n,19,8,8] (a shard's `s`) and, optionally, their `legal_mask` [n,4672] ->
    {"status": i32 [n] (0 or a DECODE_STATUS reason), "flags": i32 [n], "nlegal": i32 [n], "fens": [str] * n}.  The mask
    supplies the en-passant square (the planes have none) and is audited against the decoded position's legal moves
    (status "mask_mismatch"); without one en passant is unknown and set to none.  A FEN is empty where the status leaves no
    position.  One wave per row on the device (m0_decode_planes)."""
    pl = np.ascontiguousarray(planes, dtype=np.float32)
    if pl.ndim != 4 or pl.shape[1:] != (19, 8, 8):
        raise ValueError("planes must be [n,19,8,8]")
    n = int(pl.shape[0])
    mk = None
    if mask is not None:
        mk = np.ascontiguousarray(np.asarray(mask).reshape(n, -1), dtype=np.uint8)
        if mk.shape != (n, 4672):
            raise ValueError("mask must be [n,4672]")
    status, flags, nlegal = (np.zeros((n,), np.int32) for _ in range(3))
    stride = 96
    fens = C.create_string_buffer(max(1, n) * stride)
    if n:
        _lib.check(_lib.lib().m0_decode_planes(int(device_index), ptr(pl), ptr(mk), n, ptr(status), ptr(flags), ptr(nlegal), fens,
                                               stride), "m0_decode_planes")
    raw = fens.raw
    return {"status": status, "flags": flags, "nlegal": nlegal,
            "fens": [raw[i * stride: (i + 1) * stride].split(b"\0", 1)[0].decode() for i in range(n)]}


def encode_board(fen: str) -> np.ndarray:
    """encode_board, encoding.py:11-46 -> float32 [19,8,8]."""
    return encode_fens([fen], want_moves=False)[0][0]


def move_to_index(fen: str, uci: str) -> int:
    """move_to_index, encoding.py:114-150; ValueError for an illegal move (:120-121)."""
    out = C.c_int32(0)
    _lib.check(_lib.lib().m0_move_to_index_fen(0, fen.encode(), uci.encode(), C.byref(out)), "move_to_index")
    return int(out.value)


class MoveEncoder:
    """MoveEncoder, encoding.py:153-253 (encode_move / get_legal_actions)."""

    def encode_move(self, fen: str, uci: str) -> int:
        return move_to_index(fen, uci)

    def decode_move(self, fen: str, action_idx: int) -> str:
        """encoding.py:174-229 -> UCI string ('0000' = Move.null())."""
        if not (0 <= int(action_idx) < 4672):
            raise ValueError("action_idx out of range")
        buf = C.create_string_buffer(8)
        _lib.check(_lib.lib().m0_decode_move_fen(0, fen.encode(), int(action_idx), buf), "decode_move")
        return buf.value.decode()

    def get_legal_actions(self, fen: str) -> np.ndarray:
        return encode_fens([fen], want_moves=False)[1][0]


def build_horizontal_flip_permutation() -> np.ndarray:
    """encoding.py:310-347: E<->W, NE<->NW, SE<->SW per step; knight pairs; under-promo left/right."""
    perm = list(range(73))
    for step in range(7):
        for a, b in ((2, 3), (4, 5), (6, 7)):
            perm[a * 7 + step], perm[b * 7 + step] = perm[b * 7 + step], perm[a * 7 + step]
    for off in (0, 2, 4, 6):
        perm[56 + off], perm[57 + off] = perm[57 + off], perm[56 + off]
    for blk in (64, 67, 70):
        perm[blk + 1], perm[blk + 2] = perm[blk + 2], perm[blk + 1]
    return np.ascontiguousarray(perm, dtype=np.int64)


def build_rotate180_permutation() -> np.ndarray:
    """encoding.py:350-386: N<->S, E<->W, NE<->SW, NW<->SE per step; knight 180 pairs; under-promo l/r."""
    perm = list(range(73))
    for step in range(7):
        for a, b in ((0, 1), (2, 3), (4, 7), (5, 6)):
            perm[a * 7 + step], perm[b * 7 + step] = perm[b * 7 + step], perm[a * 7 + step]
    for a, b in ((56, 63), (57, 62), (58, 61), (59, 60)):
        perm[a], perm[b] = perm[b], perm[a]
    for blk in (64, 67, 70):
        perm[blk + 1], perm[blk + 2] = perm[blk + 2], perm[blk + 1]
    return np.ascontiguousarray(perm, dtype=np.int64)


def augment_kinds(kind, n: int) -> np.ndarray:
    """`kind` as the u8 [n] the library reads: a name of AUGMENT_KINDS for every row, or one kind (0, 1, 2) per row."""
    if isinstance(kind, str):
        if kind not in AUGMENT_KINDS:
            raise ValueError(f"augmentation must be one of {sorted(AUGMENT_KINDS)} or an array of kinds, got {kind!r}")
        return np.full((n,), AUGMENT_KINDS[kind], np.uint8)
    raw = np.asarray(kind)
    if raw.shape != (n,) or raw.dtype.kind not in "iub" or ((raw < 0) | (raw > max(AUGMENT_KINDS.values()))).any():
        raise ValueError(f"per-row augmentation kinds must be [{n}] integers in 0..{max(AUGMENT_KINDS.values())}")
    return np.ascontiguousarray(raw, dtype=np.uint8)


def augment(s, pi, legal_mask=None, kind="hflip", device_index: int = 0):
    """The trainer's augmentation of rows (train.py:280-305): s f32 [n,P,8,8], pi f32 [n,4672], legal_mask [n,4672] or None ->
    (s', pi', legal_mask') of the same shapes (legal_mask' u8, or None), transformed on the device (m0_augment_rows,
    include/m0_augment.h).  kind: "hflip" (files mirrored, build_horizontal_flip_permutation on the move types), "rot180" (ranks
    and files, build_rotate180_permutation), "none" (a copy), or one kind of AUGMENT_KINDS' values per row.  Values travel as their
    bits.  This is the trainer's transform, not a symmetry of chess: see DESIGN.md section 8."""
    a = np.ascontiguousarray(s, dtype=np.float32)
    if a.ndim != 4 or a.shape[2:] != (8, 8) or a.shape[1] <= 0:
        raise ValueError(f"expected planes [n,P,8,8], got {a.shape}")
    n = int(a.shape[0])
    p = np.ascontiguousarray(pi, dtype=np.float32)
    if p.shape != (n, LEGACY_POLICY_SIZE):
        raise ValueError(f"expected pi [{n},{LEGACY_POLICY_SIZE}], got {p.shape}")
    m = None
    if legal_mask is not None:
        m = np.ascontiguousarray(np.asarray(legal_mask).reshape(n, -1), dtype=np.uint8)
        if m.shape != p.shape:
            raise ValueError(f"expected legal_mask [{n},{LEGACY_POLICY_SIZE}], got {m.shape}")
    kinds = augment_kinds(kind, n)
    s_out, pi_out = np.empty_like(a), np.empty_like(p)
    m_out = None if m is None else np.empty_like(m)
    if n:
        _lib.check(_lib.lib().m0_augment_rows(int(device_index), ptr(a), int(a.shape[1]), ptr(p), ptr(m), ptr(kinds), n, ptr(s_out),
                                              ptr(pi_out), ptr(m_out)), "m0_augment_rows")
    return s_out, pi_out, m_out
