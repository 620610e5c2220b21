"""The float64 reference of the SSL score (include/m0_ssl_score.h): the reference's SSL losses (azchess/model/resnet.py:892-1130)
restated per row in numpy float64 -- log-sum-exp cross-entropies, binary cross-entropy with logits on clamped targets, the
control thresholds -- plus the count columns and flags as the header defines them.  Targets of planes come from the oracle's
own generator (oracle/ssl_ref.py), not from the code under test.  `mutate` names one deliberate error
(tests/test_ssl_score.py checks that the case set sees each of them)."""
import numpy as np

from matrix0_amd import _abi
from oracle import ssl_ref

COLS = _abi.SSL_SCORE_COLS
TASKS = tuple(_abi.SSL_BITS)
CHANNELS = {"piece": 13, "threat": 1, "pin": 1, "fork": 1, "control": 3}
MUTATIONS = ("control_threshold_at_zero", "bce_target_not_clamped", "control_channels_shifted")
LOSS_COLUMNS, EXACT_COLUMNS = tuple(range(5)), tuple(range(5, 16))


def bits(tasks):
    return sum(_abi.SSL_BITS[t] for t in tasks)


def names(tasks_bits):
    return [t for t in TASKS if tasks_bits & _abi.SSL_BITS[t]]


def usable(row):
    """the header's rule for one row of planes [19,8,8]"""
    p, side = row[:12], row[12]
    with np.errstate(invalid="ignore"):
        return bool(((p == 0) | (p == 1)).all() and (p == 1).sum(axis=0).max() <= 1 and (side == side.flat[0]).all()
                    and side.flat[0] in (0.0, 1.0))


def pack(t):
    """the oracle's maps of one position as [17,64]"""
    return np.concatenate([t["piece"].reshape(13, 64)] + [t[k].reshape(1, 64) for k in TASKS[1:]]).astype(np.float64)


def targets_planes(planes):
    """(float64 [B,17,64], zero where the row is not usable; usable bool [B])"""
    planes = np.asarray(planes, np.float32).reshape(-1, 19, 8, 8)
    ok = np.array([usable(r) for r in planes])
    return np.stack([pack(ssl_ref.targets(r)) if u else np.zeros((17, 64)) for r, u in zip(planes, ok)]), ok


def _classes(t, mutate=None):
    """[B,5,64] integer classes of a [B,17,64] target array: piece 0..12, the three binary maps, control 0..2"""
    lo, hi = (0.0, 0.0) if mutate == "control_threshold_at_zero" else (-0.5, 0.5)
    control = np.where(t[:, 16] < lo, 0, np.where(t[:, 16] > hi, 2, 1))
    return np.stack([np.argmax(t[:, :13], axis=1)] + [(t[:, 13 + k] >= 0.5).astype(np.int64) for k in range(3)] + [control], axis=1)


def _cross_entropy(z, cls):
    """z [B,N,64], cls [B,64] -> (loss [B,64], arg-max hit [B,64])"""
    m = z.max(axis=1, keepdims=True)
    lse = np.log(np.exp(z - m).sum(axis=1)) + m[:, 0]
    return lse - np.take_along_axis(z, cls[:, None], axis=1)[:, 0], np.argmax(z, axis=1) == cls


def score_rows(heads, tasks, planes, targets=None, mutate=None):
    """float64 [B,16]; tasks: the bitmask"""
    assert mutate is None or mutate in MUTATIONS
    task_names = names(tasks)
    B = len(planes)
    h = np.asarray(heads, np.float32).astype(np.float64).reshape(B, -1, 64)
    assert h.shape[1] == sum(CHANNELS[t] for t in task_names)
    own, ok = targets_planes(planes)
    stored = targets is not None
    t = np.asarray(targets, np.float32).astype(np.float64).reshape(B, 17, 64) if stored else own
    cls = _classes(t, mutate)
    out = np.zeros((B, COLS))
    flags = np.where(ok, 0, 1)
    if stored:
        differ = (_classes(t) != _classes(own))[:, [TASKS.index(k) for k in task_names]].any(axis=(1, 2))
        flags = flags | np.where(ok & differ, 4, 0)
    flags = flags | np.where(np.isfinite(h).all(axis=(1, 2)), 0, 2)
    h = np.nan_to_num(h, nan=0.0, posinf=0.0, neginf=0.0)          # flagged rows are zeroed below
    off = 0
    for name in task_names:
        k = TASKS.index(name)
        if name == "control" and mutate == "control_channels_shifted" and off > 0:
            off -= 1
        z = h[:, off:off + CHANNELS[name]]
        off += CHANNELS[name]
        if name == "piece":
            loss, hit = _cross_entropy(z, cls[:, 0])
            occupied = cls[:, 0] != 12
            out[:, 5], out[:, 6], out[:, 7] = hit.sum(axis=1), (hit & occupied).sum(axis=1), occupied.sum(axis=1)
        elif name == "control":
            loss, hit = _cross_entropy(z, cls[:, 4])
            out[:, 14] = hit.sum(axis=1)
        else:
            z, raw = z[:, 0], t[:, 12 + k]
            tc = raw if mutate == "bce_target_not_clamped" else np.clip(raw, 0.0, 1.0)
            loss = np.maximum(z, 0) - z * tc + np.log1p(np.exp(-np.abs(z)))
            if name != "pin":
                says, actual = z > 0, cls[:, k] == 1
                c = 8 if name == "threat" else 11
                out[:, c], out[:, c + 1], out[:, c + 2] = (says & actual).sum(axis=1), says.sum(axis=1), actual.sum(axis=1)
        out[:, k] = loss.mean(axis=1)
    zero = ((flags & 2) != 0) | (((flags & 1) != 0) & (not stored))
    out[zero, :15] = 0.0
    out[:, 15] = flags
    return out


def tolerance(ref):
    """|got - ref| <= 1e-4 * (1 + |ref|), the project's rule for fp32 sums (tests/score_ref.py): here a sum of 64 squares merged
    in six steps, each term good to a few 2^-24 relative (the core's own exp and log are within about 2 ulp), so the rule leaves a
    margin of more than ten."""
    return 1e-4 * (1.0 + np.abs(ref))


def compare(got, ref):
    """The largest error per column as a multiple of its tolerance (<= 1 passes); columns 5-15 must be equal (inf if not)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all() and np.isfinite(ref).all()
    worst = (np.abs(got - ref) / tolerance(ref)).max(axis=0)
    for c in EXACT_COLUMNS:
        worst[c] = 0.0 if np.array_equal(got[:, c], ref[:, c]) else np.inf
    return worst
