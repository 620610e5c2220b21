"""The SSL target maps of a batch on the device (include/m0_batch_ssl.h): the SSL instantiation of batch_rows_kernel through
m0_rowstore_batch_ssl against the host call (which tests/test_device_replay_ssl.py compares with the independent oracle) and
against m0_ssl_targets_planes on the planes the same call returned; rows across segments and after an eviction; torch tensors
filled on a side stream; the score kernel fed with the batch's maps; and the launch without maps beside it.  Every comparison is
of bit patterns; nothing here has a tolerance."""
import numpy as np
import pytest

from matrix0_amd import _abi, _lib, device_replay as dr, rowpack as rp
from tests import rowpack_cases as rc
from tests.test_device_replay import same
from tests.test_device_replay_ssl import batch_ssl_host, canaries6, raw_batch_ssl, untouched

pytestmark = pytest.mark.gpu

BATCHES = (1, 3, 5, 65, 257)       # one row per wave: the sizes of tests/test_device_replay_gpu.py


def edge(B, with_mask):
    s, pi, z, mask = rc.edge_rows(B, seed=B, with_mask=with_mask)[:4]
    return rp.pack_rows(s, pi, z, mask, device="host")


def from_torch(tensors):
    import torch
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in tensors]


def targets_planes(planes):
    """m0_ssl_targets_planes: (maps f32 [n,17,8,8], zero where the call left them alone; status i32 [n])"""
    planes = np.ascontiguousarray(planes, np.float32)
    out, status = np.zeros((len(planes), 17, 8, 8), np.float32), np.full(len(planes), -1, np.int32)
    rcode = _lib.lib().m0_ssl_targets_planes(0, _lib.ptr(planes), len(planes), _lib.ptr(out), _lib.ptr(status))
    assert rcode == _abi.M0_OK, _lib.last_error()
    return out, status


@pytest.mark.parametrize("with_mask", (True, False), ids=("mask", "nomask"))
@pytest.mark.parametrize("B", BATCHES)
def test_the_kernel_equals_the_host_call_and_the_targets_of_its_own_planes(B, with_mask):
    packed = edge(B, with_mask)
    rows, kinds = np.arange(B), np.arange(B) % 3
    want = [w for w in batch_ssl_host(packed, rows, kinds) if w is not None]
    with dr.DeviceReplay(0, with_mask) as store:
        assert store.append(packed) == range(B)
        got = store.batch(rows, kinds, ssl=True)                                       # host pointers
        assert not same(got, want)
        assert not same(from_torch(store.batch_torch(rows, kinds, ssl=True)), want)    # device pointers, read back
        assert not same(store.batch(rows[::-1], kinds[::-1], ssl=True), [w[::-1] for w in want])
    maps, status = targets_planes(got[0])
    assert rc.same_bits(got[-1], status)
    assert rc.same_bits(got[-2], maps)                                                 # zero where the status is 1
    assert not got[-2][status == 1].view(np.uint32).any()
    if B >= 65:
        assert status.any() and not status.all()


def test_the_en_passant_rows_under_every_kind():
    s, pi, z, mask = rc.ep_rows()[:4]
    packed = rp.pack_rows(s, pi, z, mask, device="host")
    rows, kinds = np.tile(np.arange(13), 3), np.repeat([0, 1, 2], 13)
    with dr.DeviceReplay(0) as store:
        store.append(packed)
        got = store.batch(rows, kinds, ssl=True)
    assert not same(got, batch_ssl_host(packed, rows, kinds))
    assert not got[5].any() and rc.same_bits(got[4], targets_planes(got[0])[0])
    assert not rc.same_bits(got[4][26:], got[4][:13][..., ::-1, ::-1])                 # the maps of rotated planes, not rotated maps


def test_rows_gathered_across_segments_and_after_an_eviction():
    s, pi, z, mask = rc.edge_rows(94, seed=3)[:4]
    packed = rp.pack_rows(s, pi, z, mask, device="host")
    parts = [packed.rows(0, 40), packed.rows(40, 70), packed.rows(70, 94)]
    assert all(p.kinds()["rows"]["raw"] >= 1 for p in parts)
    rng = np.random.default_rng(11)
    rows = np.concatenate([rng.integers(0, 94, size=56), [0, 0, 39, 40, 69, 70, 93, 93]])
    kinds = rng.integers(0, 3, size=64)
    want = batch_ssl_host(packed, rows, kinds)
    assert want[5].any()
    with dr.DeviceReplay(0) as store:
        for p in parts:
            store.append(p)
        assert not same(store.batch(rows, kinds, ssl=True), want)
        store.evict(keep_rows=50)
        stay = rows >= 40
        assert 0 < stay.sum() < 64
        assert not same(store.batch(rows[stay], kinds[stay], ssl=True), [w[stay] for w in want])
        out = canaries6(64)
        assert raw_batch_ssl(store, rows, kinds, out) == _lib.M0_ERR_INVALID and untouched(out)
        assert str(int(rows[~stay][0])) in _lib.last_error()
        assert raw_batch_ssl(store, rows, np.full(64, 3), out) == _lib.M0_ERR_INVALID and untouched(out)
        assert raw_batch_ssl(store, rows[stay], kinds[stay], out[:4] + [None, out[5]]) == _lib.M0_ERR_INVALID and untouched(out)
        assert raw_batch_ssl(store, rows[stay], kinds[stay], out[:5] + [None]) == _lib.M0_ERR_INVALID and untouched(out)
        # a new segment after the eviction: ids go on, old rows stay where they were
        assert store.append(parts[0]) == range(94, 134)
        again = np.concatenate([rows[stay], [94, 133]])
        k2 = np.concatenate([kinds[stay], [1, 2]])
        want2 = batch_ssl_host(packed, np.concatenate([rows[stay], [0, 39]]), k2)
        assert not same(store.batch(again, k2, ssl=True), want2)


def test_a_rows_maps_do_not_depend_on_its_place_or_on_the_batch():
    packed = edge(257, True)
    five, five_kinds = np.array([3, 10, 14, 100, 256]), np.array([1, 2, 1, 0, 2])            # two RAW rows among them
    assert packed.fields["row_kind"][[3, 14]].tolist() == [rc.RAW, rc.RAW]
    with dr.DeviceReplay(0) as store:
        store.append(packed)
        alone = store.batch(five, five_kinds, ssl=True)
        assert not same(alone, batch_ssl_host(packed, five, five_kinds))
        assert sorted(alone[5].tolist()) == [0, 0, 0, 0, 1]                                   # row 3 is the 0.5 in a piece plane
        assert not same(store.batch(five, five_kinds, ssl=True), alone)                       # a repetition
        for B, at in ((5, [4, 3, 2, 1, 0]), (65, [0, 13, 32, 63, 64]), (257, [256, 255, 128, 1, 0])):
            rows, kinds = (np.arange(B) * 7) % 257, np.arange(B) % 3
            rows[at], kinds[at] = five, five_kinds
            got = store.batch(rows, kinds, ssl=True)
            assert not same([g[at] for g in got], alone), B


def test_batch_torch_fills_the_maps_on_the_current_stream():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no device")
    packed = edge(65, True)
    rows, kinds = np.arange(65)[::-1].copy(), np.arange(65) % 3
    with dr.DeviceReplay(0) as store:
        store.append(packed)
        want = store.batch(rows, kinds, ssl=True)
        side = torch.cuda.Stream(device=0)
        with torch.cuda.stream(side):
            out = store.batch_torch(rows, kinds, ssl=True)
        side.synchronize()
        assert [tuple(t.shape) for t in out] == [(65, 19, 8, 8), (65, 4672), (65,), (65, 4672), (65, 17, 8, 8), (65,)]
        assert [t.dtype for t in out] == [torch.float32, torch.float32, torch.float32, torch.uint8, torch.float32, torch.int32]
        assert all(t.device == torch.device("cuda", 0) for t in out)
        assert not same([t.cpu().numpy() for t in out], want)
        # the given storage is written again
        ptrs = [t.data_ptr() for t in out]
        for t in out:
            t.fill_(5)
        with torch.cuda.stream(side):
            again = store.batch_torch(rows, kinds, out=out, ssl=True)
        side.synchronize()
        assert [t.data_ptr() for t in again] == ptrs and not same([t.cpu().numpy() for t in out], want)
        with pytest.raises(ValueError):
            store.batch_torch(rows[:5], kinds[:5], out=out, ssl=True)
        with pytest.raises(ValueError):
            store.batch_torch(rows, kinds, out=out[:4], ssl=True)                     # the list without maps
        with pytest.raises(ValueError):
            store.batch_torch(rows, kinds, out=out)                                   # ... and the longer one without ssl
        # the dictionary over tensors: views of the tensor
        t = dr.ssl_targets(out[4])
        assert tuple(t["piece"].shape) == (65, 13, 8, 8) and tuple(t["control"].shape) == (65, 8, 8)
        assert t["piece"].data_ptr() == out[4].data_ptr() and t["threat"].data_ptr() == out[4][:, 13].data_ptr()
        # the iterator hands the same tensors' worth
        s, pi, z, mask, ssl, status, ids, kind = next(store.batches(16, epochs=1, seed=2, torch=True, ssl=True))
        torch.cuda.synchronize()
        assert not same([x.cpu().numpy() for x in (s, pi, z, mask, ssl, status)], store.batch(ids, kind, ssl=True))


def test_the_score_kernel_reads_the_batchs_maps_as_it_reads_the_planes():
    s, pi, z, mask = (a[:65] for a in rc.worker_rows())
    packed = rp.pack_rows(s, pi, z, mask, device="host")
    rows, kinds = np.arange(65), (np.arange(65) % 3).astype(np.uint8)
    with dr.DeviceReplay(0) as store:
        store.append(packed)
        planes, _, _, _, ssl, status = store.batch(rows, kinds, ssl=True)
    assert not status.any()
    tasks = sum(_abi.SSL_BITS.values())
    heads = (np.random.default_rng(21).standard_normal((65, 19, 64)) * 3).astype(np.float32)
    out = []
    for targets in (np.ascontiguousarray(ssl.reshape(65, 17, 64)), None):
        got = np.full((65, _abi.SSL_SCORE_COLS), -7, np.float32)
        rcode = _lib.lib().m0_ssl_score_rows(0, _lib.ptr(heads), tasks, _lib.ptr(planes), _lib.ptr(targets), 65, _lib.ptr(got))
        assert rcode == _abi.M0_OK, _lib.last_error()
        out.append(got)
    assert rc.same_bits(out[0], out[1])
    flags = out[0][:, 15].astype(np.int64)
    assert not (flags & _abi.SSL_SCORE_FLAGS["mismatch"]).any() and not flags.any()
    assert (out[0][:, :5] > 0).all()                                                   # all five tasks were scored


def test_the_batch_without_maps_is_still_what_it_was():
    for with_mask in (True, False):
        packed = edge(65, with_mask)
        rows, kinds = (np.arange(65) * 7) % 65, np.arange(65) % 3
        with dr.DeviceReplay(0, with_mask) as store:
            store.append(packed)
            plain = store.batch(rows, kinds)
            full = store.batch(rows, kinds, ssl=True)
            assert len(plain) == len(full) - 2 == (4 if with_mask else 3)
            assert not same(plain, full[:len(plain)])
            assert not same(store.batch(rows, kinds), plain)                           # and after a launch with maps as before
