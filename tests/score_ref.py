"""The float64 reference of the training-loss score (include/m0_score.h): the reference trainer's loss
(azchess/training/train.py:436-549) restated per row in torch float64 with its own expressions -- torch.where(mask, p, -1e9),
log_softmax, smooth_l1_loss, mse_loss -- plus the rank, entropy and mass columns as the header defines them.  `mutate` names one
deliberate error (tests/test_score.py checks that the case set sees each of them)."""
import numpy as np
import torch
from torch.nn import functional as F

COLS = 8
MUTATIONS = ("no_target_union", "smooth_all_columns", "fp32_softmax_without_max", "huber_delta_ignored", "rank_ge",
             "tie_highest_index")


def score_rows(logits, value, pi, z, mask=None, *, mask_mode="legal", label_smoothing=0.0, value_loss="mse", huber_delta=1.0,
               mutate=None):
    """float64 ndarray [B, 8]"""
    assert mutate is None or mutate in MUTATIONS
    p = torch.as_tensor(np.asarray(logits, np.float32)).double()
    v = torch.as_tensor(np.asarray(value, np.float32)).double()
    pi = torch.as_tensor(np.asarray(pi, np.float32)).double()
    z = torch.as_tensor(np.asarray(z, np.float32)).double()
    B, n_cols = p.shape
    eps = float(label_smoothing)
    flags = torch.zeros(B, dtype=torch.int64)

    if mask_mode == "legal":
        legal = torch.as_tensor(np.asarray(mask)).bool()
        # train.py:210-217, per row: a target that sums to <= 0 becomes uniform over the legal moves
        uniform = (pi.sum(dim=1) <= 0) & legal.any(dim=1)
        flags |= uniform.long() * 4
        pi = torch.where(uniform[:, None], legal.double() / legal.sum(dim=1, keepdim=True).clamp_min(1), pi)
        support = legal if mutate == "no_target_union" else legal | (pi > 0)          # :444-449
        smooth_set = support
    elif mask_mode == "target":
        support = pi > 0                                                               # apply_policy_mask, :82
        smooth_set = support
    else:
        support = torch.ones_like(pi, dtype=torch.bool)                                # :460
        smooth_set = pi > 0                                                            # :512
    empty = ~support.any(dim=1)
    nonfinite = ~torch.isfinite(p).all(dim=1) | ~torch.isfinite(v)
    flags |= empty.long() * 1 | nonfinite.long() * 2
    v = torch.nan_to_num(v, nan=0.0, posinf=0.0, neginf=0.0)                           # :536-538
    p = torch.nan_to_num(p, nan=0.0, posinf=0.0, neginf=0.0)                           # flagged rows are zeroed below

    p_for_loss = torch.where(support, p, torch.full_like(p, -1e9))                     # :449
    if mutate == "fp32_softmax_without_max":
        e = torch.exp(p_for_loss.float())
        log_probs = torch.log(e / e.sum(dim=1, keepdim=True)).double()
    else:
        log_probs = F.log_softmax(p_for_loss, dim=1)                                   # :505
    if eps > 0.0:                                                                      # :506-516
        if mutate == "smooth_all_columns":
            smooth_set = torch.ones_like(smooth_set)
        counts = smooth_set.sum(dim=1, keepdim=True).clamp_min(1)
        pi_smooth = (1.0 - eps) * pi + eps * smooth_set.double() / counts.double()
    else:
        pi_smooth = pi
    # a masked column's product is 0 * -1e9 = 0 in the reference; its pi_smooth is 0 here as well
    policy = -(torch.where(pi_smooth > 0, pi_smooth * log_probs, torch.zeros_like(p))).sum(dim=1)
    entropy = -(torch.where(pi_smooth > 0, pi_smooth * torch.log(pi_smooth.clamp_min(1e-300)), torch.zeros_like(p))).sum(dim=1)

    if value_loss == "huber":                                                          # :546-549
        beta = 1.0 if mutate == "huber_delta_ignored" else float(huber_delta)
        vloss = F.smooth_l1_loss(v, z, beta=beta, reduction="none")
    else:
        vloss = F.mse_loss(v, z, reduction="none")

    best = pi.max(dim=1, keepdim=True).values
    index = torch.arange(n_cols).expand(B, n_cols)
    if mutate == "tie_highest_index":
        target = torch.where(pi == best, index, torch.full_like(index, -1)).max(dim=1).values
    else:
        target = torch.where(pi == best, index, torch.full_like(index, n_cols)).min(dim=1).values
    target_logit = p.gather(1, target[:, None])
    above = (p >= target_logit) if mutate == "rank_ge" else (p > target_logit)
    rank = (above & support).sum(dim=1).double()
    mass = (torch.softmax(p, dim=1) * support.double()).sum(dim=1)                     # :476-478, as its complement

    out = torch.stack([policy, entropy, vloss, rank, mass, support.sum(dim=1).double(), v, flags.double()], dim=1)
    out[:, :5] = torch.where((empty | nonfinite)[:, None], torch.zeros_like(out[:, :5]), out[:, :5])
    return out.numpy()


def tolerance(ref):
    """|got - ref| <= 1e-4 * (1 + |ref|): fp32 sums of about 73 terms per lane and six merges stay below 80 * 2^-24 = 5e-6
    relative, the terms (logit - max - lse, all of one sign) are exact to 2^-24, so this leaves a margin of about ten."""
    return 1e-4 * (1.0 + np.abs(ref))


EXACT_COLUMNS = (3, 5, 7)


def compare(got, ref):
    """The largest error per column as a multiple of its tolerance (<= 1 passes); columns 3, 5 and 7 must be equal (inf if not)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all() and np.isfinite(ref).all()
    worst = (np.abs(got - ref) / tolerance(ref)).max(axis=0)
    for c in EXACT_COLUMNS:
        worst[c] = 0.0 if np.array_equal(got[:, c], ref[:, c]) else np.inf
    return worst
