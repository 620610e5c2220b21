"""The seeded case set of the SSL score tests (CPU: the host build against the float64 reference; GPU: the kernel against the host
build, bit for bit).  A group is one task set with head outputs, planes and, for the stored variants, targets; its rows are
named after what they are there for."""
import functools

import numpy as np

from tests import ssl_score_ref as ref

TASK_SETS = {"all": ("piece", "threat", "pin", "fork", "control"), "piece": ("piece",), "piece_control": ("piece", "control")}


def _board(rng, fill, white):
    """planes [19,8,8] of a random board: each square holds one of the 12 pieces with probability `fill`"""
    p = np.zeros((19, 8, 8), np.float32)
    for sq in np.flatnonzero(rng.random(64) < fill):
        p[rng.integers(12), sq // 8, sq % 8] = 1.0
    p[12] = 1.0 if white else 0.0
    p[13:17] = rng.integers(0, 2, size=(4, 1, 1))
    p[17], p[18] = rng.random() * 0.5, rng.random()
    return p


def _rows(seed, channels):
    """names, heads [n,C,64], planes [n,19,8,8]"""
    rng = np.random.default_rng(seed)
    names, heads, planes = [], [], []

    def add(name, p, h=None, scale=3.0):
        names.append(name)
        planes.append(p)
        heads.append((rng.standard_normal((channels, 64)) * scale).astype(np.float32) if h is None else h.astype(np.float32))

    for k, fill in enumerate((0.4, 0.5, 0.25, 0.6, 0.1, 0.45)):
        add(f"random board {k}", _board(rng, fill, k % 2 == 0))
    add("empty board", _board(rng, 0.0, True))
    add("every square occupied", _board(rng, 1.1, False))
    add("logits up to +-40", _board(rng, 0.4, True), scale=16.0)
    big = np.where(rng.random((channels, 64)) < 0.5, 40.0, -40.0)
    add("logits of exactly +-40", _board(rng, 0.4, False), big)
    add("equal logits: the arg-max is the lowest index", _board(rng, 0.4, True), np.zeros((channels, 64)))
    two = (rng.standard_normal((channels, 64)) * 2).astype(np.float32)
    two[1] = two[0]
    add("two equal leading channels", _board(rng, 0.5, False), two)
    nan = (rng.standard_normal((channels, 64)) * 3).astype(np.float32)
    nan[channels - 1, 63] = np.nan
    add("a NaN head output", _board(rng, 0.4, True), nan)
    inf = (rng.standard_normal((channels, 64)) * 3).astype(np.float32)
    inf[0, 0] = np.inf
    add("an infinite head output", _board(rng, 0.4, False), inf)
    p = _board(rng, 0.4, True)
    p[3].flat[np.flatnonzero(p[:12].sum(axis=0).reshape(-1) == 0)[0]] = 0.5
    add("unusable: 0.5 in a piece plane", p)
    p = _board(rng, 0.4, False)
    sq = np.flatnonzero(p[:12].sum(axis=0).reshape(-1) == 1)[0]
    p[(int(np.argmax(p[:12].reshape(12, 64)[:, sq])) + 5) % 12].flat[sq] = 1.0
    add("unusable: two pieces on one square", p)
    p = _board(rng, 0.4, True)
    p[12, 7, 7] = 0.0
    add("unusable: plane 12 not uniform", p)
    p = _board(rng, 0.4, True)
    p[12] = 2.0
    add("unusable: plane 12 is 2 everywhere", p)
    return names, np.stack(heads), np.stack(planes)


def _stored(seed, planes):
    """targets [n,17,64] for the rows: the planes' own (the oracle's), then by row number modulo 6: 0 as they are, 1 all zero,
    2 values beyond [0, 1] and soft control values in the same classes, 3 one square moved to another class, 4 soft piece
    channels with the same arg-max, 5 control values near the thresholds in other classes"""
    rng = np.random.default_rng(seed)
    t, _ = ref.targets_planes(planes)
    t = t.astype(np.float32)
    for b in range(len(t)):
        kind = b % 6
        if kind == 1:
            t[b] = 0.0
        elif kind == 2:
            t[b, 13:16] = np.where(t[b, 13:16] >= 0.5, 2.0, -1.0)
            t[b, 16] = np.where(t[b, 16] < -0.5, -0.7, np.where(t[b, 16] > 0.5, 0.6, rng.choice([-0.4, 0.3], size=64)))
        elif kind == 3:
            t[b, 15, 5] = 1.0 - t[b, 15, 5]
        elif kind == 4:
            t[b, :13] = t[b, :13] * 0.5 + 0.25
        elif kind == 5:
            t[b, 16] = rng.choice([-0.51, -0.5, -0.2, 0.2, 0.5, 0.51], size=64)
    return t


@functools.lru_cache(maxsize=None)
def groups():
    out = []
    for k, (name, tasks) in enumerate(TASK_SETS.items()):
        bits = ref.bits(tasks)
        names, heads, planes = _rows(100 + k, sum(ref.CHANNELS[t] for t in tasks))
        out.append(dict(name=f"{name}:planes", tasks=bits, names=names, heads=heads, planes=planes, targets=None))
        out.append(dict(name=f"{name}:stored", tasks=bits, names=names, heads=heads, planes=planes, targets=_stored(200 + k, planes)))
    return out


def tiled(g, B, shift=0):
    """the group's rows repeated cyclically up to B, starting at row `shift`: (heads, planes, targets), and the row numbers"""
    idx = (np.arange(B) + shift) % len(g["names"])
    take = lambda a: None if a is None else np.ascontiguousarray(a[idx])
    return (take(g["heads"]), take(g["planes"]), take(g["targets"])), idx
