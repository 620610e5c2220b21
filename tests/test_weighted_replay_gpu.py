"""The weighted row store on the device (include/m0_batch_weighted.h: csrc/sample_kernels.hip through a device store) against the
host store, which tests/test_weighted_replay.py compares with the numpy reference: the same three segments and the same weight
set on both, draws to host memory and into torch tensors, weights written from device tensors and drawn from on the same stream,
and the sampled batch against the batch of its ids.  Every comparison is of integers or bit patterns; nothing here has a
tolerance."""
import numpy as np
import pytest

from matrix0_amd import device_replay as dr, rowpack as rp
from tests import rowpack_cases as rc
from tests.test_weighted_replay import MODES, N, make_store, packed_segments, ref_sample, same_bits, ticks, weight_set

pytestmark = pytest.mark.gpu

SIZES = (1, 64, 257)


def cpu(tensors):
    import torch
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in tensors]


@pytest.fixture(scope="module")
def stores():
    w = weight_set()
    with make_store(0, w) as dev, make_store("host", w) as host:
        yield dev, host


def test_weights_and_sums_are_the_host_stores(stores):
    dev, host = stores
    assert same_bits(dev.weights(np.arange(N)), host.weights(np.arange(N)))
    assert same_bits(dev.weights([N - 1, 0, 0, 1024, 2024]), weight_set()[[N - 1, 0, 0, 1024, 2024]])
    assert dev.weights_info() == host.weights_info()
    assert dev.weights_info()["total_ticks"] == int(ticks(weight_set()).sum(dtype=np.uint64))
    with make_store(0) as fresh:                                         # weight 1 from the first weighted call
        assert fresh.weights_info() == {"total_ticks": N << 24, "rows_with_ticks": N, "sanitised_or_skipped": 0, "degenerate_draws": 0}


@pytest.mark.parametrize("stratified", MODES, ids=("independent", "stratified"))
@pytest.mark.parametrize("B", SIZES + (1000,))
def test_a_draw_is_the_host_stores_to_host_memory_and_through_tensors(stores, B, stratified):
    dev, host = stores
    for seed, draw in ((0, 0), (12345, (7 << 32) | 9)):
        want_ids, want_prob = host.sample(B, seed, draw, stratified)
        ids, prob = dev.sample(B, seed, draw, stratified)
        assert ids.tolist() == want_ids.tolist() and same_bits(prob, want_prob)
        ids, prob = cpu(dev.sample(B, seed, draw, stratified, torch=True))
        assert ids.tolist() == want_ids.tolist() and same_bits(prob, want_prob)
    assert same_bits(want_prob, ref_sample(weight_set(), 0, B, 12345, (7 << 32) | 9, stratified)[1])


@pytest.mark.parametrize("ssl", (False, True), ids=("plain", "ssl"))
@pytest.mark.parametrize("stratified", MODES, ids=("independent", "stratified"))
@pytest.mark.parametrize("B", SIZES)
def test_a_sampled_batch_is_the_host_stores_and_the_batch_of_its_ids(stores, B, stratified, ssl):
    dev, host = stores
    kinds = np.arange(B) % 3
    want = host.sampled_batch(B, 8, B, kinds, stratified, ssl)
    got = dev.sampled_batch(B, 8, B, kinds, stratified, ssl)                               # host pointers
    assert len(got) == len(want) == (8 if ssl else 6) and all(same_bits(a, b) for a, b in zip(got, want))
    tensors = dev.sampled_batch(B, 8, B, kinds, stratified, ssl, torch=True)               # device pointers, nothing waited for
    again = dev.batch_torch(tensors[-2].cpu().numpy(), kinds, ssl=ssl)
    assert all(same_bits(a, b) for a, b in zip(cpu(tensors), want))
    assert all(same_bits(a, b) for a, b in zip(cpu(tensors[:-2]), cpu(again)))
    out = dev.sampled_batch(B, 8, B + 1, kinds, stratified, ssl, torch=True, out=tensors[:-2])
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(out, tensors[:-2]))
    assert all(same_bits(a, b) for a, b in zip(cpu(out), host.sampled_batch(B, 8, B + 1, kinds, stratified, ssl)))


def test_a_store_without_masks():
    w = weight_set()
    with make_store(0, w, with_mask=False) as dev, make_store("host", w, with_mask=False) as host:
        want = host.sampled_batch(65, 2, 2, 1, True, True)
        assert len(want) == 7 and all(same_bits(a, b) for a, b in zip(dev.sampled_batch(65, 2, 2, 1, True, True), want))
        assert all(same_bits(a, b) for a, b in zip(cpu(dev.sampled_batch(65, 2, 2, 1, True, True, torch=True)), want))


def test_weights_from_device_tensors_are_sanitised_counted_and_seen_by_the_next_draw_on_the_stream():
    import torch
    w = weight_set()
    ids = np.array([3, 1500, 2061, 40, N + 5, 41, 1023, 1024, -1], np.int64)
    values = np.array([np.nan, 5.0, -2.0, np.inf, 1.0, 70000.0, 0.5, 2.0 ** -25, 9.0], np.float32)
    clean = np.array([0.0, 5.0, 0.0, 65536.0, 0.0, 65536.0, 0.5, 2.0 ** -25, 0.0], np.float32)
    resident = (ids >= 0) & (ids < N)
    with make_store(0, w) as dev, make_store("host", w) as host:
        host.set_weights(ids[resident], clean[resident])
        before = dev.sample(257, 6, 6)[0]
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            tid, tval = torch.from_numpy(ids).cuda(), torch.from_numpy(values).cuda()
            dev.set_weights(tid, tval)                                   # enqueued ...
            drawn = dev.sample(257, 6, 6, torch=True)                    # ... and drawn from behind it, with no wait between
            batch = dev.sampled_batch(64, 6, 7, 2, torch=True)
        stream.synchronize()
        want_ids, want_prob = host.sample(257, 6, 6)
        assert drawn[0].cpu().numpy().tolist() == want_ids.tolist() and same_bits(drawn[1].cpu().numpy(), want_prob)
        assert before.tolist() != want_ids.tolist()
        assert all(same_bits(a.cpu().numpy(), b) for a, b in zip(batch, host.sampled_batch(64, 6, 7, 2)))
        assert same_bits(dev.weights(np.arange(N)), host.weights(np.arange(N)))
        got, want = dev.weights_info(), host.weights_info()
        assert got["sanitised_or_skipped"] == 4 + 2 and want["sanitised_or_skipped"] == 0      # NaN, -2, inf, 70000; two ids outside
        assert {k: v for k, v in got.items() if k != "sanitised_or_skipped"} == {k: v for k, v in want.items() if k != "sanitised_or_skipped"}
        # an id twice: one of the two values, and sums that are exact for it
        twice = torch.tensor([7, 7, 7, 8], dtype=torch.int64, device="cuda")
        dev.set_weights(twice, torch.tensor([1.0, 2.0, 3.0, 4.0], device="cuda"))
        seven = float(dev.weights([7])[0])
        assert seven in (1.0, 2.0, 3.0)
        host.set_weights([7, 8], [seven, 4.0])
        assert dev.weights_info()["total_ticks"] == host.weights_info()["total_ticks"]
        assert dev.sample(64, 1, 1, True)[0].tolist() == host.sample(64, 1, 1, True)[0].tolist()
        with pytest.raises(ValueError):
            dev.set_weights(twice.cpu(), torch.ones(4))                  # tensors of another device
        with pytest.raises(ValueError):
            host.set_weights(twice, torch.ones(4, device="cuda"))


def test_fill_scale_append_and_evict_on_the_device():
    w = weight_set()
    with make_store(0, w) as dev, make_store("host", w) as host:
        for s in (dev, host):
            s.fill_weights(range(990, 1030), 65536.0)
            s.scale_weights(0.37)
            assert s.append(packed_segments()[2]) == range(N, N + 37)
            s.fill_weights(range(N, N + 37), 7.0)
            s.evict(1025 + 37 + 37)
        w[990:1030] = 65536.0
        w = np.concatenate([w * np.float32(0.37), np.full(37, 7.0, np.float32)]).astype(np.float32)
        keep = np.arange(1000, N + 37)
        assert dev.info()["first_row"] == 1000
        assert same_bits(dev.weights(keep), w[1000:]) and same_bits(host.weights(keep), w[1000:])
        assert dev.weights_info() == host.weights_info()
        for stratified in MODES:
            ids, prob = dev.sample(257, 3, 3, stratified)
            want = ref_sample(w[1000:], 1000, 257, 3, 3, stratified)
            assert ids.tolist() == want[0].tolist() and same_bits(prob, want[1]) and ids.min() >= 1000
        got = dev.sampled_batch(65, 3, 4, 1)
        assert all(same_bits(a, b) for a, b in zip(got, host.sampled_batch(65, 3, 4, 1)))
        with pytest.raises(ValueError, match="999"):
            dev.set_weights([999], [1.0])
        # nothing to draw from: uniform, inside the window, counted
        for s in (dev, host):
            s.scale_weights(0.0)
        ids, prob = dev.sample(257, 1, 1)
        want = host.sample(257, 1, 1)
        assert ids.tolist() == want[0].tolist() and same_bits(prob, want[1]) and ids.min() >= 1000 and ids.max() < N + 37
        got = cpu(dev.sampled_batch(64, 1, 2, 0, torch=True))
        assert all(same_bits(a, b) for a, b in zip(got, host.sampled_batch(64, 1, 2, 0)))
        assert dev.weights_info() == host.weights_info() and dev.weights_info()["degenerate_draws"] == 2


def test_more_blocks_than_one_pass_of_the_prefix_takes():
    """1030 segments of two rows are 1030 blocks: the block prefix takes two passes of 1024, and the segment table has grown"""
    s, pi, z, mask = rc.edge_rows(2, seed=3)[:4]
    two = rp.pack_rows(s, pi, z, mask, device="host")
    w = np.random.default_rng(5).gamma(0.5, 2.0, 2060).astype(np.float32)
    with dr.DeviceReplay(0) as dev:
        dev.append(two)
        dev.set_weights([0, 1], w[:2])                                   # weighted from the first segment on: every append adds its entry
        for _ in range(1029):
            dev.append(two)
        dev.set_weights(np.arange(2, 2060), w[2:])
        assert dev.weights_info()["total_ticks"] == int(ticks(w).sum(dtype=np.uint64))
        for stratified in MODES:
            ids, prob = dev.sample(257, 2, 2, stratified)
            want = ref_sample(w, 0, 257, 2, 2, stratified)
            assert ids.tolist() == want[0].tolist() and same_bits(prob, want[1])
        assert ids.max() >= 2048
        got = dev.sampled_batch(65, 2, 3, 2)
        assert all(same_bits(a, b) for a, b in zip(got, dev.batch(got[-2], 2)))


# ---- scoring resident rows, and their loss as their weight ----
SMALL = dict(planes=19, channels=64, blocks=2, attention_heads=4, policy_size=4672, norm="group", activation="silu", preact=True,
             policy_factor_rank=32, self_supervised=False)


@pytest.fixture(scope="module")
def small_net():
    from matrix0_amd.backend import M0Backend
    from tests import net_layer_cases as net_cases
    be = M0Backend.from_state_dict(SMALL, net_cases.weights(SMALL, sharp=True))
    yield be
    be.close()


def test_score_resident_is_the_score_of_the_packed_rows_and_of_the_augmented_rows(small_net):
    packed = packed_segments()[2]                                        # 37 rows, ids 2025 ..
    dense = rp.unpack_rows(packed, device="host")
    ids = np.arange(N - 37, N)
    with make_store(0, weight_set()) as dev:
        for opts in (dict(), dict(mask_mode="target", value_loss="huber", huber_delta=0.7, label_smoothing=0.05), dict(mask_mode="none")):
            want = small_net.score(packed=packed, **opts)
            assert same_bits(small_net.score_resident(dev, ids, **opts), want), opts
            back = small_net.score_resident(dev, ids[::-1], **opts)
            assert same_bits(back, small_net.score(*[d[::-1] for d in dense], **opts)), opts
        kinds = np.arange(37) % 3
        assert same_bits(small_net.score_resident(dev, ids, kinds), small_net.score(*dense, augment=kinds.astype(np.uint8)))
        assert same_bits(small_net.score_resident(dev, ids, 1), small_net.score(*dense, augment="hflip"))
        assert same_bits(dev.weights(np.arange(N)), weight_set())        # no rule: no weight moves
        with pytest.raises(ValueError, match=str(N)):
            small_net.score_resident(dev, [N])
    with make_store("host") as host, pytest.raises(ValueError, match="host"):
        small_net.score_resident(host, ids)
    with make_store(0, with_mask=False) as bare:
        with pytest.raises(ValueError, match="legal_mask"):
            small_net.score_resident(bare, ids, mask_mode="legal")
        want = small_net.score(packed=packed_segments(False)[2], mask_mode="target")
        assert same_bits(small_net.score_resident(bare, ids), want)      # without masks the mode is "target"


def test_a_rule_turns_the_scored_rows_loss_into_their_weights_on_the_device(small_net):
    w = weight_set()
    ids = np.concatenate([np.arange(990, 1030)[::-1], [0, N - 1, 2024]])  # distinct, over two segments and three blocks
    with make_store(0, w) as dev, make_store("host", w) as host:
        for rule in (dr.weight_rule(1.0, 0.0, 0.0, 1e-3, 65536.0), dr.weight_rule(0.5, 2.0, -3.0, 0.25, 4.0),
                     dr.weight_rule(0.0, 0.0, 0.0, 0.0, 0.0)):
            rows = small_net.score_resident(dev, ids, rule=rule)
            assert same_bits(rows, small_net.score_resident(dev, ids))   # the columns do not change with a rule
            want = dr.weight_from_score(rows, rule)
            assert same_bits(dev.weights(ids), want)
            w[ids] = want
            assert same_bits(dev.weights(np.arange(N)), w)               # rows outside ids keep their weights
            host.set_weights(ids, want)
            assert dev.weights_info() == host.weights_info()
            assert dev.sample(257, 2, 2)[0].tolist() == host.sample(257, 2, 2)[0].tolist()
        with pytest.raises(ValueError):
            small_net.score_resident(dev, ids, rule=dr.weight_rule(cap=65537.0))
        with pytest.raises(ValueError):
            small_net.score_resident(dev, ids, rule=dr.weight_rule(floor=-1.0))
        assert same_bits(dev.weights(np.arange(N)), w)
        # every resident row, in id order
        rule = dr.weight_rule(1.0, 0.0, 0.5, 1e-3, 16.0)
        means = dev.reweigh(small_net, rule, batch_size=700)
        rows = np.concatenate([small_net.score_resident(dev, np.arange(a, min(a + 700, N))) for a in range(0, N, 700)])
        assert same_bits(dev.weights(np.arange(N)), dr.weight_from_score(rows, rule)) and means["rows"] == N
        # the means of the rule's inputs (the edge rows hold pi entries that are not numbers: their policy loss is none either);
        # 2062 float64 additions in another order differ by less than 2062 * 2^-53 of a sum of positive terms
        want = rows[:, :3].sum(axis=0, dtype=np.float64) / N
        assert np.allclose([means["policy_loss"], means["entropy"], means["value_loss"]], want, rtol=1e-12, atol=0, equal_nan=True)
        assert np.isfinite(want[2]) and want[2] > 0
