"""The trainer's augmentation restated in numpy (azchess/training/train.py:284-305): np.flip where it calls torch.flip, fancy
indexing where it calls index_select, driven by the two permutations the reference's own functions returned
(tests/golden/ref_augment_perm.json, written by tools/gen_golden_augment_perm.py).  Shared by the CPU and the GPU tests."""
import functools
import json
import os

import numpy as np

NONE, HFLIP, ROT180 = 0, 1, 2
KINDS = {"none": NONE, "hflip": HFLIP, "rot180": ROT180}
POLICY_SHAPE = (8, 8, 73)
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_augment_perm.json")


@functools.lru_cache(maxsize=None)
def perms():
    """{HFLIP: i64 [73], ROT180: i64 [73]} as the reference built them"""
    with open(FIXTURE) as f:
        d = json.load(f)
    out = {HFLIP: np.array(d["horizontal_flip"], np.int64), ROT180: np.array(d["rotate180"], np.int64)}
    assert all(p.shape == (73,) for p in out.values())
    return out


def _uniform(s, pi, mask, kind):
    if kind == NONE:
        return s.copy(), pi.copy(), None if mask is None else mask.copy()
    # train.py:286-294 (dims [3] and [2]) and :297-305 (dims [2, 3] and [1, 2])
    s_axes, pi_axes = ((3,), (2,)) if kind == HFLIP else ((2, 3), (1, 2))
    perm = perms()[kind]
    n = len(pi)
    move = lambda a: np.ascontiguousarray(np.flip(a.reshape(n, *POLICY_SHAPE), axis=pi_axes)[..., perm]).reshape(n, -1)
    return np.ascontiguousarray(np.flip(s, axis=s_axes)), move(pi), None if mask is None else move(mask)


def augment(s, pi, mask, kind):
    """(s', pi', mask') for s [B,P,8,8], pi [B,4672], mask [B,4672] or None; kind a name, a number, or one number per row.  The
    arrays keep their types and their bits."""
    s, pi = np.asarray(s), np.asarray(pi)
    mask = None if mask is None else np.asarray(mask)
    if isinstance(kind, str):
        kind = KINDS[kind]
    if np.ndim(kind) == 0:
        return _uniform(s, pi, mask, int(kind))
    kinds = np.asarray(kind)
    assert kinds.shape == (len(s),)
    s_out, pi_out = np.empty_like(s), np.empty_like(pi)
    m_out = None if mask is None else np.empty_like(mask)
    for k in (NONE, HFLIP, ROT180):
        rows = np.flatnonzero(kinds == k)
        if len(rows):
            a, b, c = _uniform(s[rows], pi[rows], None if mask is None else mask[rows], k)
            s_out[rows], pi_out[rows] = a, b
            if mask is not None:
                m_out[rows] = c
    return s_out, pi_out, m_out
