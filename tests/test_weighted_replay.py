"""The weighted row store on the CPU (include/m0_batch_weighted.h, matrix0_amd/device_replay.py; no GPU): a host store against a
reference of a dozen lines of numpy and Python integers -- ticks, np.cumsum in uint64, searchsorted(side="right"), mix64.  Ids
and counts are compared as integers, weights and probabilities as bit patterns; nothing here has a tolerance.  The one bound
(the distribution test) is a condition on the rule, worked out below."""
import functools

import numpy as np
import pytest

from matrix0_amd import device_replay as dr, rowpack as rp
from tests import rowpack_cases as rc

U64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
SEGMENTS = (1000, 1025, 37)     # blocks of 1024 rows from a segment's first row: an edge inside a segment, a block of one row at a
N = sum(SEGMENTS)               # segment's end, and a segment smaller than a block
MODES = (False, True)
SIZES = (1, 7, 64, 257, 1000)


# ---- the reference ----
def mix64(x):
    x ^= x >> 30
    x = x * 0xBF58476D1CE4E5B9 & U64
    x ^= x >> 27
    x = x * 0x94D049BB133111EB & U64
    return x ^ x >> 31


def ticks(w):
    return (np.asarray(w, np.float32) * np.float32(2 ** 24)).astype(np.uint64)


def ref_sample(w, first, B, seed, draw, stratified):
    """(ids, prob) of a draw over rows first .. first + len(w) - 1 with these weights"""
    t = ticks(w)
    S = np.cumsum(t, dtype=np.uint64)
    total = int(S[-1])
    key = mix64(mix64((seed + G) & U64) ^ (draw * 0xD6E8FEB86659FD93 & U64))
    ids, prob = np.empty(B, np.int64), np.empty(B, np.float32)
    for b in range(B):
        x = mix64((key + (b + 1) * G) & U64)
        if total == 0:
            ids[b], prob[b] = first + (x * len(w) >> 64), np.float32(1.0 / len(w))
            continue
        q, rem = divmod(total, B)
        span = q + (b < rem)
        r = b * q + min(b, rem) + (x * span >> 64) if stratified and span else x * total >> 64
        i = int(np.searchsorted(S, np.uint64(r), side="right"))
        ids[b], prob[b] = first + i, np.float32(float(t[i]) / float(total))
    return ids, prob


def weight_set(seed=7):
    """f32 [N]: gamma-distributed weights and every edge of the format and of the block layout"""
    w = np.random.default_rng(seed).gamma(0.5, 2.0, N).astype(np.float32)
    w[5], w[6], w[7], w[8] = 0.0, 2.0 ** -25, 2.0 ** -24, 65536.0        # no ticks, no ticks, one tick, the maximum
    w[1000:2024] = 0.0                                                   # a whole block: the first of the second segment
    w[[0, 999, 2025, N - 1]] = 0.0                                       # the first and the last row of a block
    assert ticks(w[6:8]).tolist() == [0, 1] and (w >= 0).all() and w.max() == 65536.0
    return w


@functools.lru_cache(maxsize=None)
def packed_segments(with_mask=True):
    out = []
    for k, n in enumerate(SEGMENTS):
        s, pi, z, mask = rc.edge_rows(n, seed=k, with_mask=with_mask)[:4]
        out.append(rp.pack_rows(s, pi, z, mask, device="host"))
    return tuple(out)


def make_store(device="host", weights=None, with_mask=True, segments=None):
    store = dr.DeviceReplay(device, with_mask)
    for p in (packed_segments(with_mask) if segments is None else segments):
        store.append(p)
    if weights is not None:
        store.set_weights(np.arange(len(weights)), weights)
    return store


def same_bits(a, b):
    return rc.same_bits(np.asarray(a), np.asarray(b))


def small_store(n, device="host"):
    """A store of the first n rows of the first segment's source rows"""
    s, pi, z, mask = rc.edge_rows(n, seed=0)[:4]
    store = dr.DeviceReplay(device)
    store.append(rp.pack_rows(s, pi, z, mask, device="host"))
    return store


# ---- the draw ----
@pytest.fixture(scope="module")
def store():
    with make_store(weights=weight_set()) as s:
        yield s


def test_a_store_gets_weight_one_at_its_first_weighted_call_and_keeps_its_sums():
    with make_store() as s:
        assert s.weights_info() == {"total_ticks": N << 24, "rows_with_ticks": N, "sanitised_or_skipped": 0, "degenerate_draws": 0}
        assert same_bits(s.weights(np.arange(N)), np.ones(N, np.float32))
        assert s.append(packed_segments()[2]) == range(N, N + 37)        # an append of a weighted store: weight 1 too
        assert s.weights_info()["total_ticks"] == (N + 37) << 24
        w = weight_set()
        s.set_weights(np.arange(N), w)
        assert same_bits(s.weights(np.arange(N)), w)
        i = s.weights_info()
        assert i["total_ticks"] == int(ticks(w).sum(dtype=np.uint64)) + (37 << 24)
        assert i["rows_with_ticks"] == int((ticks(w) > 0).sum()) + 37


@pytest.mark.parametrize("stratified", MODES, ids=("independent", "stratified"))
@pytest.mark.parametrize("B", SIZES)
def test_a_draw_equals_the_numpy_reference_id_for_id_and_prob_bit_for_bit(store, B, stratified):
    w = weight_set()
    for seed, draw in ((0, 0), (12345, 3), (U64, (7 << 32) | 9)):
        ids, prob = store.sample(B, seed, draw, stratified)
        want_ids, want_prob = ref_sample(w, 0, B, seed, draw, stratified)
        assert ids.tolist() == want_ids.tolist(), (seed, draw)
        assert same_bits(prob, want_prob), (seed, draw)
        assert (ticks(w)[ids] > 0).all()


@pytest.mark.parametrize("B", SIZES)
def test_stratified_ids_ascend_and_every_row_gets_its_share(store, B):
    t = ticks(weight_set()).astype(object)
    total = int(t.sum())
    ids, _ = store.sample(B, 99, 1, True)
    assert (np.diff(ids) >= 0).all()
    counts = np.bincount(ids, minlength=N)
    for i in range(N):
        assert B * int(t[i]) // total - 1 <= counts[i] <= -(-B * int(t[i]) // total) + 1, i


def test_independent_draws_follow_the_weights():
    """200 draws of 1000 over 50 rows: every row's count within 5 binomial standard deviations of 200 000 p, rows without ticks
    never drawn.  The numpy model of this rule reaches 2.6 standard deviations on such a set; 5 is a condition, passed by a
    sound generator with probability 1 - 50 * 6e-7."""
    w = np.random.default_rng(1).gamma(0.5, 2.0, 50).astype(np.float32)
    w[[3, 17, 49]] = 0.0
    w[4] = 2.0 ** -25
    with small_store(50) as s:
        s.set_weights(np.arange(50), w)
        counts = np.zeros(50, np.int64)
        for draw in range(200):
            counts += np.bincount(s.sample(1000, 12345, draw)[0], minlength=50)
    t = ticks(w).astype(np.float64)
    p = t / t.sum()
    n = 200 * 1000
    assert counts.sum() == n and not counts[t == 0].any() and (t == 0).sum() == 4
    sd = np.sqrt(n * p * (1 - p))
    worst = np.abs(counts - n * p)[t > 0] / sd[t > 0]
    assert worst.max() <= 5.0, worst.max()


def test_one_row_with_all_the_weight_and_a_store_with_none():
    w = np.zeros(50, np.float32)
    w[31] = 2.0 ** -24                                                   # one tick in all
    with small_store(50) as s:
        s.set_weights(np.arange(50), w)
        for stratified in MODES:
            ids, prob = s.sample(64, 5, 0, stratified)
            assert (ids == 31).all() and (prob == 1.0).all()
        assert s.weights_info() == {"total_ticks": 1, "rows_with_ticks": 1, "sanitised_or_skipped": 0, "degenerate_draws": 0}
        # nothing to draw from: uniform over the resident rows, and counted
        s.fill_weights(range(0, 50), 0.0)
        for k, stratified in enumerate(MODES):
            ids, prob = s.sample(257, 5, 1, stratified)
            want_ids, want_prob = ref_sample(np.zeros(50), 0, 257, 5, 1, stratified)
            assert ids.tolist() == want_ids.tolist() and same_bits(prob, want_prob) and same_bits(prob[0], np.float32(1 / 50))
            assert len(set(ids.tolist())) > 40 and ids.min() >= 0 and ids.max() < 50
            assert s.weights_info()["degenerate_draws"] == k + 1
        got = s.sampled_batch(8, 5, 2, kinds=2)
        assert s.weights_info()["degenerate_draws"] == 3
        assert all(same_bits(a, b) for a, b in zip(got, s.batch(got[-2], 2)))


# ---- writes ----
def test_refusals_change_nothing():
    w = weight_set()
    with make_store(weights=w) as s:
        before = s.weights_info()
        bad = [([N], [1.0]), ([-1], [1.0]), ([3, 4, 3], [1.0, 1.0, 1.0]), ([3, 4], [1.0, np.nan]), ([3, 4], [1.0, -1e-30]),
               ([3, 4], [1.0, 65536.01]), ([3, 4], [np.inf, 1.0])]
        for ids, values in bad:
            with pytest.raises(ValueError):
                s.set_weights(ids, values)
        with pytest.raises(ValueError, match=str(N)):
            s.set_weights([3, N], [2.0, 2.0])
        for r, v in ((range(N - 1, N + 1), 1.0), (range(-1, 3), 1.0), (range(0, 3), np.nan), (range(0, 3), 65537.0), (range(0, 3), -1.0)):
            with pytest.raises(ValueError):
                s.fill_weights(r, v)
        for f in (-1.0, np.nan, np.inf):
            with pytest.raises(ValueError):
                s.scale_weights(f)
        with pytest.raises(ValueError):
            s.weights([0, N])
        assert same_bits(s.weights(np.arange(N)), w) and s.weights_info() == before
        # an evicted id is refused by every call that names ids
        s.evict(N - 1000)
        assert s.info()["first_row"] == 1000
        for call in (lambda: s.set_weights([999], [1.0]), lambda: s.weights([999]), lambda: s.fill_weights(range(999, 1001), 1.0)):
            with pytest.raises(ValueError, match="999"):
                call()
        assert same_bits(s.weights(np.arange(1000, N)), w[1000:])


def test_weights_survive_an_append_and_an_eviction_and_no_draw_names_an_evicted_row():
    w = weight_set()
    with make_store(weights=w) as s:
        assert s.append(packed_segments()[2]) == range(N, N + 37)
        w2 = np.concatenate([w, np.ones(37, np.float32)])
        assert same_bits(s.weights(np.arange(N + 37)), w2)
        s.evict(1025 + 37 + 37)
        assert s.info()["first_row"] == 1000 and s.info()["segments"] == 3
        assert same_bits(s.weights(np.arange(1000, N + 37)), w2[1000:])
        assert s.weights_info()["total_ticks"] == int(ticks(w2[1000:]).sum(dtype=np.uint64))
        for stratified in MODES:
            ids, prob = s.sample(257, 4, 4, stratified)
            want_ids, want_prob = ref_sample(w2[1000:], 1000, 257, 4, 4, stratified)
            assert ids.tolist() == want_ids.tolist() and same_bits(prob, want_prob) and ids.min() >= 1000
        got = s.sampled_batch(64, 4, 5, kinds=np.arange(64) % 3)
        assert got[-2].min() >= 1000 and all(same_bits(a, b) for a, b in zip(got, s.batch(got[-2], np.arange(64) % 3)))
        s.evict(0)
        with pytest.raises(ValueError):
            s.sample(4, 0, 0)
        assert s.weights_info()["total_ticks"] == 0


def test_fill_and_scale_are_numpy_float32():
    w = weight_set()
    with make_store(weights=w) as s:
        for lo, hi, v in ((990, 1010, 65536.0), (1023, 1025, 0.25), (2024, 2030, 2.0 ** -24), (0, N, 3.0), (5, 5, 9.0)):
            s.fill_weights(range(lo, hi), v)
            w[lo:hi] = v
            assert same_bits(s.weights(np.arange(N)), w)
            assert s.weights_info()["total_ticks"] == int(ticks(w).sum(dtype=np.uint64))
        w = weight_set()
        s.set_weights(np.arange(N), w)
        for f in (0.99, 1e-3, 70000.0, 123.456, 0.0):
            s.scale_weights(f)
            w = np.minimum(np.float32(65536.0), w * np.float32(f)).astype(np.float32)
            assert same_bits(s.weights(np.arange(N)), w), f
            i = s.weights_info()
            assert i["total_ticks"] == int(ticks(w).sum(dtype=np.uint64)) and i["rows_with_ticks"] == int((ticks(w) > 0).sum())
            ids, prob = s.sample(64, 1, 1)
            want = ref_sample(w, 0, 64, 1, 1, False)
            assert ids.tolist() == want[0].tolist() and same_bits(prob, want[1])


# ---- batches ----
@pytest.mark.parametrize("with_mask", (True, False), ids=("mask", "nomask"))
def test_a_sampled_batch_is_the_batch_of_the_ids_it_returns(with_mask):
    w = weight_set()
    with make_store(weights=w, with_mask=with_mask) as s:
        for B, stratified, ssl in ((1, False, False), (65, True, False), (65, False, True), (257, True, True)):
            kinds = np.arange(B) % 3
            got = s.sampled_batch(B, 21, B, kinds, stratified, ssl)
            ids, prob = got[-2:]
            want = ref_sample(w, 0, B, 21, B, stratified)
            assert ids.tolist() == want[0].tolist() and same_bits(prob, want[1])
            assert same_bits(ids, s.sample(B, 21, B, stratified)[0])
            ref = s.batch(ids, kinds, ssl=ssl)
            assert len(got) == len(ref) + 2 and all(same_bits(a, b) for a, b in zip(got, ref)), (B, stratified, ssl)
        none = s.sampled_batch(7, 1, 1)                                  # no kinds: untransformed
        assert all(same_bits(a, b) for a, b in zip(none, s.batch(none[-2])))
        with pytest.raises(ValueError):
            s.sampled_batch(4, 1, 1, kinds=[0, 1, 2, 3])
        with pytest.raises(ValueError):
            s.sampled_batch(4, 1, 1, torch=True)                         # a host store has no device outputs


def test_weighted_batches_are_a_function_of_seed_epoch_and_index():
    w = weight_set()
    with make_store(weights=w) as s:
        runs = [list(s.batches(500, epochs=2, seed=3, weighted=True, stratified=st)) for st in (False, False, True)]
        assert len(runs[0]) == 2 * (N // 500)
        for a, b in zip(runs[0], runs[1]):
            assert len(a) == 7 and all(same_bits(x, y) for x, y in zip(a, b))
        assert any(not same_bits(a[4], b[4]) for a, b in zip(runs[0], runs[2]))
        plan_kinds = [int(k) for e in range(2) for k in s.plan(e, 500, 3)[1]]
        for n, got in enumerate(runs[0]):
            e, j = divmod(n, N // 500)
            assert got[5] == plan_kinds[n]
            alone = s.sampled_batch(500, 3, (e << 32) | j, got[5])
            assert all(same_bits(x, y) for x, y in zip(got[:5] + (got[6],), alone))
            assert same_bits(got[4], ref_sample(w, 0, 500, 3, (e << 32) | j, False)[0])
        assert not same_bits(runs[0][0][4], runs[0][N // 500][4])        # another epoch, another draw


def test_the_unweighted_iterator_does_not_see_the_weights():
    with make_store(weights=weight_set()) as weighted, make_store() as plain:
        a = list(weighted.batches(300, epochs=1, seed=9))
        b = list(plain.batches(300, epochs=1, seed=9))
        assert len(a) == len(b) == N // 300
        for x, y in zip(a, b):
            assert len(x) == len(y) == 6 and x[5] == y[5] and all(same_bits(p, q) for p, q in zip(x[:5], y[:5]))


# ---- the loss of a row as its weight ----
def ref_weight(rows, rule):
    """The float32 formula: each fused step in float64 (the product of two float32 is exact there), rounded to float32"""
    f32, f64 = np.float32, np.float64
    c0, c1, c2 = (rows[:, k].astype(f32) for k in range(3))
    t = np.full(len(rows), rule.floor, f32)
    for a, x in ((rule.policy, c0), (rule.kl, (c0 - c1).astype(f32)), (rule.value, c2)):
        t = (f64(f32(a)) * x.astype(f64) + t.astype(f64)).astype(f32)
    with np.errstate(invalid="ignore"):
        t = np.where(t > 0, t, f32(0)).astype(f32)
    return np.minimum(t, f32(rule.cap)).astype(f32)


def test_weight_from_score_is_the_float32_formula():
    rng = np.random.default_rng(11)
    rows = np.zeros((4096, 8), np.float32)
    rows[:, 0] = rng.gamma(2.0, 1.5, 4096)            # policy loss
    rows[:, 1] = rng.gamma(2.0, 0.5, 4096)            # entropy of the target
    rows[:, 2] = rng.random(4096) * 4                 # value loss
    rows[:, 3:7] = rng.random((4096, 4))
    rows[7] = 0.0                                     # a flagged row: zero columns, flag 1
    rows[7, 7] = 1.0
    rows[8, :3] = (1e30, 0.0, 1e30)                   # beyond the cap
    rows[9, :3] = (0.0, 1e30, 0.0)                    # far below zero under a kl term
    rules = [dr.weight_rule(), dr.weight_rule(1.0, 0.0, 0.0, 1e-3, 65536.0), dr.weight_rule(0.5, 2.0, -3.0, 0.25, 4.0),
             dr.weight_rule(-1.0, 0.0, 0.0, 0.0, 1.0), dr.weight_rule(3.0, 1.5, 0.75, 2.0 ** -24, 100.0)]
    for rule in rules:
        got = dr.weight_from_score(rows, rule)
        assert same_bits(got, ref_weight(rows, rule)), [rule.policy, rule.kl, rule.value, rule.floor, rule.cap]
        assert same_bits(got[7], np.float32(rule.floor)) and got.min() >= 0 and got.max() <= rule.cap
    assert dr.weight_from_score(rows, rules[1])[8] == 65536.0 and dr.weight_from_score(rows, rules[2])[9] == 0.0
    for bad in (dict(floor=-1e-9), dict(cap=65536.5), dict(cap=-1.0), dict(policy=np.nan), dict(kl=np.inf), dict(value=-np.inf)):
        with pytest.raises(ValueError):
            dr.weight_from_score(rows, dr.weight_rule(**bad))
    with pytest.raises(ValueError):
        dr.weight_from_score(rows[:, :7], rules[0])
