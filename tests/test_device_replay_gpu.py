"""The resident row store on the device (include/m0_batch.h, matrix0_amd/device_replay.py): batch_rows_kernel through
m0_rowstore_batch against m0_rowstore_batch_host (which tests/test_device_replay.py compares with unpack-then-augment in numpy)
and against the existing device chain m0_rowpack_unpack -> m0_augment_rows; rows gathered across segments and after an eviction;
torch tensors filled on a side stream; and M0Backend.score of a batch against the score under the same augmentation.  Every
comparison is of bit patterns; nothing here has a tolerance."""
import functools

import numpy as np
import pytest

from matrix0_amd import _lib, device_replay as dr, encoding, rowpack as rp
from tests import net_layer_cases as net_cases
from tests import rowpack_cases as rc
from tests.test_device_replay import batch_host, canaries, raw_batch, same, untouched
from tests.test_rowpack_gpu import SMALL

pytestmark = pytest.mark.gpu

BATCHES = (1, 3, 5, 65, 257)       # one row per wave: a partial workgroup, whole ones and a partial last one for 2 .. 8 rows a workgroup


def chain(packed, rows, kinds):
    """The existing device path: m0_rowpack_unpack of the rows, then m0_augment_rows"""
    s, pi, z, mask = rp.unpack_rows(packed, device=0)
    rows = np.asarray(rows)
    a, b, c = encoding.augment(s[rows], pi[rows], None if mask is None else mask[rows], np.asarray(kinds, np.uint8))
    return a, b, z[rows], c


def from_torch(tensors):
    import torch
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in tensors]


@functools.lru_cache(maxsize=None)
def edge(B, with_mask):
    s, pi, z, mask = rc.edge_rows(B, seed=B, with_mask=with_mask)[:4]
    return rp.pack_rows(s, pi, z, mask, device="host")


@pytest.mark.parametrize("with_mask", (True, False), ids=("mask", "nomask"))
@pytest.mark.parametrize("B", BATCHES)
def test_the_kernel_equals_the_host_call_and_the_chain(B, with_mask):
    packed = edge(B, with_mask)
    rows, kinds = np.arange(B), np.arange(B) % 3
    want = [w for w in batch_host(packed, rows, kinds) if w is not None]
    with dr.DeviceReplay(0, with_mask) as store:
        assert store.append(packed) == range(B)
        got = store.batch(rows, kinds)                                         # host pointers
        assert not same(got, want)
        assert not same(got, [c for c in chain(packed, rows, kinds) if c is not None])
        assert not same(from_torch(store.batch_torch(rows, kinds)), want)      # device pointers, read back
        assert not same(store.batch(rows[::-1], kinds[::-1]), [w[::-1] for w in want])


def test_the_en_passant_rows_under_every_kind():
    s, pi, z, mask = rc.ep_rows()[:4]
    packed = rp.pack_rows(s, pi, z, mask, device="host")
    assert packed.kinds()["masks"]["legal"] == 13
    rows = np.tile(np.arange(13), 3)
    kinds = np.repeat([0, 1, 2], 13)
    with dr.DeviceReplay(0) as store:
        store.append(packed)
        got = store.batch(rows, kinds)
    assert not same(got, batch_host(packed, rows, kinds))
    assert not same(got, chain(packed, rows, kinds))
    assert not rc.same_bits(got[3][13:26], got[3][:13])                        # and the flip moved something


@pytest.mark.parametrize("kind", (0, 1, 2))
def test_the_worker_rows_under_a_uniform_kind_equal_the_chain(kind):
    s, pi, z, mask = rc.worker_rows()
    packed = rp.pack_rows(s, pi, z, mask, device="host")
    with dr.DeviceReplay(0) as store:
        store.append(packed)
        got = store.batch(np.arange(375), kind)
    a, b, c = encoding.augment(s, pi, mask, np.full(375, kind, np.uint8))
    assert not same(got, (a, b, z, c))


def test_rows_gathered_across_segments_and_after_an_eviction():
    s, pi, z, mask = rc.edge_rows(94, seed=3)[:4]
    packed = rp.pack_rows(s, pi, z, mask, device="host")
    parts = [packed.rows(0, 40), packed.rows(40, 70), packed.rows(70, 94)]
    assert all(p.kinds()["rows"]["raw"] >= 1 for p in parts)
    rng = np.random.default_rng(11)
    rows = np.concatenate([rng.integers(0, 94, size=56), [0, 0, 39, 40, 69, 70, 93, 93]])
    kinds = rng.integers(0, 3, size=64)
    want = batch_host(packed, rows, kinds)
    with dr.DeviceReplay(0) as store:
        for p in parts:
            store.append(p)
        assert (store.info()["segments"], store.info()["raw_rows"]) == (3, packed.kinds()["rows"]["raw"])
        assert not same(store.batch(rows, kinds), want)
        store.evict(keep_rows=50)
        assert store.resident_ids().tolist() == list(range(40, 94))
        stay = rows >= 40
        assert 0 < stay.sum() < 64
        assert not same(store.batch(rows[stay], kinds[stay]), [w[stay] for w in want])
        out = canaries(64)
        assert raw_batch(store, rows, kinds, out) == _lib.M0_ERR_INVALID and untouched(out)
        assert str(int(rows[~stay][0])) in _lib.last_error()
        assert raw_batch(store, rows[stay][:64], np.full(int(stay.sum()), 3), out) == _lib.M0_ERR_INVALID and untouched(out)
        # a new segment after the eviction: ids go on, old rows stay where they were
        assert store.append(parts[0]) == range(94, 134)
        again = np.concatenate([rows[stay], [94, 133]])
        k2 = np.concatenate([kinds[stay], [1, 2]])
        want2 = batch_host(packed, np.concatenate([rows[stay], [0, 39]]), k2)
        assert not same(store.batch(again, k2), want2)


def test_a_rows_bytes_do_not_depend_on_its_place_or_on_the_batch():
    packed = edge(257, True)
    five, five_kinds = np.array([3, 10, 14, 100, 256]), np.array([1, 2, 1, 0, 2])            # two RAW rows and the 4672-entry row among them
    f = packed.fields
    assert f["row_kind"][[3, 14]].tolist() == [rc.RAW, rc.RAW] and int(np.diff(packed.pi_off)[10]) == 4672
    with dr.DeviceReplay(0) as store:
        store.append(packed)
        alone = store.batch(five, five_kinds)
        assert not same(alone, batch_host(packed, five, five_kinds))
        assert not same(store.batch(five, five_kinds), alone)                                 # a repetition
        for B, at in ((5, [4, 3, 2, 1, 0]), (65, [0, 13, 32, 63, 64]), (257, [256, 255, 128, 1, 0])):
            rows, kinds = (np.arange(B) * 7) % 257, np.arange(B) % 3
            rows[at], kinds[at] = five, five_kinds
            got = store.batch(rows, kinds)
            assert not same([g[at] for g in got], alone), B


def test_batch_torch_fills_tensors_on_the_current_stream():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no device")
    packed = edge(65, True)
    rows, kinds = np.arange(65)[::-1].copy(), np.arange(65) % 3
    with dr.DeviceReplay(0) as store:
        store.append(packed)
        want = store.batch(rows, kinds)
        side = torch.cuda.Stream(device=0)
        with torch.cuda.stream(side):
            out = store.batch_torch(rows, kinds)
        side.synchronize()
        assert [tuple(t.shape) for t in out] == [(65, 19, 8, 8), (65, 4672), (65,), (65, 4672)]
        assert [t.dtype for t in out] == [torch.float32, torch.float32, torch.float32, torch.uint8]
        assert all(t.device == torch.device("cuda", 0) for t in out)
        assert not same([t.cpu().numpy() for t in out], want)
        # the given storage is written again
        ptrs = [t.data_ptr() for t in out]
        for t in out:
            t.zero_()
        with torch.cuda.stream(side):
            again = store.batch_torch(rows[:65], kinds, out=out)
        side.synchronize()
        assert [t.data_ptr() for t in again] == ptrs and not same([t.cpu().numpy() for t in out], want)
        with pytest.raises(ValueError):
            store.batch_torch(rows[:5], kinds[:5], out=out)
        # the iterator hands the same tensors' worth
        s, pi, z, mask, ids, kind = next(store.batches(16, epochs=1, seed=2, torch=True))
        torch.cuda.synchronize()
        assert not same([t.cpu().numpy() for t in (s, pi, z, mask)], store.batch(ids, kind))


@pytest.fixture(scope="module")
def small_net():
    from matrix0_amd.backend import M0Backend
    be = M0Backend.from_state_dict(SMALL, net_cases.weights(SMALL, sharp=True))
    yield be
    be.close()


def test_the_score_of_a_batch_is_the_score_under_the_same_augmentation(small_net):
    s, pi, z, mask = (a[:65] for a in rc.worker_rows())
    packed = rp.pack_rows(s, pi, z, mask, device="host")
    rows, kinds = np.arange(65), (np.arange(65) % 3).astype(np.uint8)
    with dr.DeviceReplay(0) as store:
        store.append(packed)
        bs, bpi, bz, bmask = store.batch(rows, kinds)
    got = small_net.score(bs, bpi, bz, bmask, mask_mode="legal")
    want = small_net.score(s, pi, z, mask, mask_mode="legal", augment=kinds)
    assert rc.same_bits(got, want), np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))
