"""The resident row store on the CPU (include/m0_batch.h, matrix0_amd/device_replay.py; no GPU): m0_rowstore_batch_host against
m0_rowpack_unpack_host followed by the numpy restatement of the trainer's augmentation, the bookkeeping of a host store, the
batch iterator and from_store.  Every comparison is of bit patterns; nothing here has a tolerance."""
import ctypes as C
import functools
import itertools
import os

import numpy as np
import pytest

from matrix0_amd import _lib, device_replay as dr, rowpack as rp
from tests import augment_ref as ar
from tests import rowpack_cases as rc


@functools.lru_cache(maxsize=None)
def case(name, with_mask):
    """(packed rows, their dense rows through m0_rowpack_unpack_host) of a named set"""
    s, pi, z, mask = rc.edge_rows(65, seed=0)[:4] if name == "edge" else rc.ep_rows()[:4]
    packed = rp.pack_rows(s, pi, z, mask if with_mask else None, device="host")
    dense = rp.unpack_rows(packed, device="host")
    assert all(rc.same_bits(a, b) for a, b in zip(dense, (s, pi, z, mask if with_mask else None)))
    return packed, dense


def batch_host(packed, rows, kinds):
    rows = np.ascontiguousarray(rows, np.int64)
    kinds = None if kinds is None else np.ascontiguousarray(kinds, np.uint8)
    B = len(rows)
    s, pi, z = np.empty((B, 19, 8, 8), np.float32), np.empty((B, 4672), np.float32), np.empty(B, np.float32)
    mask = np.empty((B, 4672), np.uint8) if packed.has_mask else None
    a = packed.c_arrays()
    rcode = _lib.lib().m0_rowstore_batch_host(C.byref(a), _lib.ptr(rows), _lib.ptr(kinds), B, _lib.ptr(s), _lib.ptr(pi), _lib.ptr(z),
                                              _lib.ptr(mask))
    assert rcode == _lib.M0_OK, _lib.last_error()
    return s, pi, z, mask


def reference(dense, rows, kinds):
    """m0_rowpack_unpack_host's rows gathered and put through tests/augment_ref.augment"""
    s, pi, z, mask = dense
    rows = np.asarray(rows)
    kinds = np.zeros(len(rows), np.int64) if kinds is None else np.asarray(kinds)
    a, b, c = ar.augment(s[rows], pi[rows], None if mask is None else mask[rows], kinds)
    return a, b, z[rows], c


def same(got, want):
    return [k for k, (g, w) in enumerate(zip(got, want)) if not rc.same_bits(g, w)]


@pytest.mark.parametrize("with_mask", (True, False), ids=("mask", "nomask"))
@pytest.mark.parametrize("name", ("edge", "ep"))
def test_the_host_batch_equals_unpack_then_augment(name, with_mask):
    packed, dense = case(name, with_mask)
    n = packed.n
    if name == "edge":
        k = packed.kinds()
        assert k["rows"]["raw"] >= 2 and (not with_mask or (k["masks"]["list"] >= 4 and k["masks"]["legal"] >= 4))
        counts = set(np.diff(packed.pi_off).tolist())
        assert set(rc.ENTRY_COUNTS) <= counts
    every = np.arange(n)
    assert not same(batch_host(packed, every, None), reference(dense, every, None))          # NULL kinds: untransformed
    for kind in (ar.NONE, ar.HFLIP, ar.ROT180):
        kinds = np.full(n, kind)
        assert not same(batch_host(packed, every, kinds), reference(dense, every, kinds)), kind
        assert not same(batch_host(packed, every[::-1], kinds), reference(dense, every[::-1], kinds)), kind
    # kinds in turn, duplicate ids
    rows = np.concatenate([every, every[::3], [0, 0, n - 1, n - 1]])
    kinds = np.arange(len(rows)) % 3
    assert not same(batch_host(packed, rows, kinds), reference(dense, rows, kinds))


@pytest.mark.parametrize("with_mask", (True, False), ids=("mask", "nomask"))
def test_a_rows_bytes_do_not_depend_on_its_place_or_on_the_batch(with_mask):
    packed, dense = case("edge", with_mask)
    n = packed.n
    for r, kind in itertools.product((0, 4, 11, 17, n - 1), (0, 1, 2)):             # PACKED and RAW rows, the 4672-entry row
        alone = batch_host(packed, [r], [kind])
        assert not same(alone, reference(dense, [r], [kind]))
        for at in (0, n // 2, n - 1):
            rows = (np.arange(n) + 7) % n
            kinds = (np.arange(n) + at) % 3
            rows[at], kinds[at] = r, kind
            got = batch_host(packed, rows, kinds)
            assert not same([None if g is None else g[at:at + 1] for g in got], alone), (r, kind, at)


def canaries(B, with_mask=True):
    out = [np.full((B, 19, 8, 8), -7, np.float32), np.full((B, 4672), -7, np.float32), np.full(B, -7, np.float32)]
    return out + ([np.full((B, 4672), 0xAB, np.uint8)] if with_mask else [])


def untouched(out):
    return all((a == (0xAB if a.dtype == np.uint8 else -7)).all() for a in out)


def raw_batch(store, rows, kinds, out):
    rows = np.ascontiguousarray(rows, np.int64)
    kinds = None if kinds is None else np.ascontiguousarray(kinds, np.uint8)
    ptrs = [_lib.ptr(a) for a in out] + [None] * (4 - len(out))
    return _lib.lib().m0_rowstore_batch(store._h, _lib.ptr(rows), _lib.ptr(kinds), len(rows), *ptrs, 0, None)


def test_a_host_store_of_three_segments_appends_evicts_and_refuses():
    s, pi, z, mask = rc.edge_rows(94, seed=3)[:4]
    packed = rp.pack_rows(s, pi, z, mask, device="host")
    dense = rp.unpack_rows(packed, device="host")
    with dr.DeviceReplay("host") as store:
        assert store.info()["rows"] == 0
        ids = [store.append(packed.rows(a, b)) for a, b in ((0, 40), (40, 70), (70, 94))]
        assert ids == [range(0, 40), range(40, 70), range(70, 94)]
        i = store.info()
        assert (i["rows"], i["first_row"], i["next_row"], i["segments"]) == (94, 0, 94, 3)
        assert i["raw_rows"] == packed.kinds()["rows"]["raw"] > 0 and 0 < i["bytes"] < i["dense_bytes"] == 94 * rp.DENSE_ROW_BYTES
        rows = np.array([93, 0, 39, 40, 69, 70, 5, 5, 41])
        kinds = np.arange(len(rows)) % 3
        assert not same(store.batch(rows, kinds), reference(dense, rows, kinds))
        store.evict(keep_rows=60)                                   # 54 would stay without the first: nothing goes
        assert store.info()["segments"] == 3
        store.evict(keep_rows=50)                                   # only the first segment goes
        i = store.info()
        assert (i["rows"], i["first_row"], i["next_row"], i["segments"]) == (54, 40, 94, 2)
        assert store.resident_ids().tolist() == list(range(40, 94))
        keep = rows[rows >= 40]
        assert not same(store.batch(keep, kinds[rows >= 40]), reference(dense, keep, kinds[rows >= 40]))
        # an evicted id, an id that never was, a kind > 2, B = 0, a missing mask: refused with the outputs as they were
        out = canaries(3)
        for bad, why in (([41, 39, 42], "39"), ([41, 94, 42], "94"), ([41, -1, 42], "-1")):
            assert raw_batch(store, bad, None, out) == _lib.M0_ERR_INVALID and why in _lib.last_error() and untouched(out)
        assert raw_batch(store, [41, 42, 43], [0, 3, 0], out) == _lib.M0_ERR_INVALID and untouched(out)
        assert raw_batch(store, [], None, out) == _lib.M0_ERR_INVALID and untouched(out)
        assert raw_batch(store, [41, 42, 43], None, out[:3]) == _lib.M0_ERR_INVALID and untouched(out)
        # device outputs of a host store
        ptrs = [_lib.ptr(a) for a in out]
        rows3 = np.array([41, 42, 43], np.int64)
        assert _lib.lib().m0_rowstore_batch(store._h, _lib.ptr(rows3), None, 3, *ptrs, 1, None) == _lib.M0_ERR_INVALID and untouched(out)
        with pytest.raises(ValueError, match="39"):
            store.batch([39])
        # the next ids go on where the last ended
        assert store.append(packed.rows(0, 2)) == range(94, 96)
        store.evict(0)
        i = store.info()
        assert (i["rows"], i["first_row"], i["next_row"], i["segments"], i["bytes"]) == (0, 96, 96, 0, 0)


def test_a_segment_of_the_other_sort_and_arrays_that_do_not_hold_together_change_nothing():
    s, pi, z, mask = rc.edge_rows(24, seed=1)[:4]
    with_masks, bare = rp.pack_rows(s, pi, z, mask, device="host"), rp.pack_rows(s, pi, z, None, device="host")
    with dr.DeviceReplay("host", with_mask=False) as store:
        store.append(bare)
        before = store.info()
        with pytest.raises(ValueError, match="mask"):
            store.append(with_masks)
        descending = rp.PackedRows(**{k: getattr(bare, k) for k in rp.ARRAY_KEYS})
        descending.pi_idx = bare.pi_idx[::-1].copy()
        with pytest.raises(ValueError, match="ascend"):
            store.append(descending)
        assert store.info() == before
        out = canaries(2, with_mask=False)
        assert raw_batch(store, [0, 1], None, out + canaries(2)[3:]) == _lib.M0_ERR_INVALID          # a superfluous mask
        got = store.batch([0, 23], [1, 2])
        assert len(got) == 3 and not same(got, reference(rp.unpack_rows(bare, device="host"), [0, 23], [1, 2])[:3])
    with dr.DeviceReplay("host", with_mask=True) as store:
        with pytest.raises(ValueError, match="mask"):
            store.append(bare)
        assert store.info()["next_row"] == 0


def test_the_kind_rule_of_the_trainer():
    table = {0.0: (1, 1), 0.4999: (1, 1), 0.5: (2, 0), 0.7499: (2, 0), 0.75: (0, 0), 0.99: (0, 0)}
    for r, (on, off) in table.items():
        assert dr.trainer_kind(r, True) == on and dr.trainer_kind(r, False) == off, r


@pytest.fixture(scope="module")
def worker_store():
    s, pi, z, mask = (a[:100] for a in rc.worker_rows())
    packed = rp.pack_rows(s, pi, z, mask, device="host")
    with dr.DeviceReplay("host") as store:
        store.append(packed.rows(0, 30))
        store.append(packed.rows(30, 100))
        store.evict(70)                                              # ids 30 .. 99 stay
        yield store, rp.unpack_rows(packed, device="host")


def test_an_epoch_visits_every_resident_row_once_in_full_batches(worker_store):
    store, dense = worker_store
    got = list(store.batches(16, epochs=2, seed=5))
    assert len(got) == 2 * (70 // 16)
    for epoch in (got[:4], got[4:]):
        ids = np.concatenate([b[4] for b in epoch])
        assert len(ids) == 64 == len(set(ids.tolist())) and set(ids.tolist()) <= set(range(30, 100))
    assert [b[4].tolist() for b in got[:4]] != [b[4].tolist() for b in got[4:]]
    kinds = {b[5] for b in store.batches(4, epochs=3, seed=5)}
    assert kinds == {0, 1, 2}
    assert {b[5] for b in store.batches(4, epochs=3, seed=5, rotate180=False)} == {0, 1}
    assert {b[5] for b in store.batches(16, epochs=1, augment="rot180")} == {2}
    for s, pi, z, mask, ids, kind in got:
        assert s.shape == (16, 19, 8, 8) and pi.shape == (16, 4672) and z.shape == (16,) and mask.shape == (16, 4672)
        assert not same((s, pi, z, mask), reference(dense, ids, np.full(16, kind)))
    with pytest.raises(ValueError):
        next(store.batches(16, augment="mirror"))
    assert list(store.batches(71, epochs=1)) == []                   # no full batch: no batch


def test_a_batch_is_a_function_of_seed_epoch_and_index(worker_store):
    store, _ = worker_store
    a, b = list(store.batches(16, epochs=2, seed=9)), list(store.batches(16, epochs=2, seed=9))
    assert len(a) == len(b) == 8
    for x, y in zip(a, b):
        assert x[5] == y[5] and not same(x[:5], y[:5])
    other = list(store.batches(16, epochs=1, seed=10))
    assert [x[4].tolist() for x in a[:4]] != [x[4].tolist() for x in other]
    # batch 2 of epoch 1, reached without consuming what comes before it
    ids, kinds = store.plan(1, 16, seed=9)
    assert ids[2].tolist() == a[4 + 2][4].tolist() and int(kinds[2]) == a[4 + 2][5]
    assert not same(store.batch(ids[2], int(kinds[2])), a[4 + 2][:4])
    skipping = store.batches(16, epochs=2, seed=9)
    sixth = next(itertools.islice(skipping, 6, None))
    assert not same(sixth[:5], a[6][:5]) and sixth[5] == a[6][5]


def test_from_store_reads_dense_and_packed_shards_and_lists_a_broken_one(tmp_path, capsys):
    from matrix0_amd.data_writer import ShardIndex, write_npz
    s, pi, z, mask = rc.worker_rows()
    os.makedirs(tmp_path / "replays")
    good = rp.pack_rows(s[40:70], pi[40:70], z[40:70], mask[40:70], device="host")
    broken = rp.packed_to_dict(good)
    broken["rowpack_pi_idx"] = broken["rowpack_pi_idx"][::-1].copy()              # columns that do not ascend
    index = ShardIndex(tmp_path)
    for name, data, rows in (("a.npz", dict(s=s[:40], pi=pi[:40], z=z[:40].reshape(-1, 1), legal_mask=mask[:40].reshape(40, 73, 8, 8)), 40),
                             ("b.npz", broken, 30), ("c.npz", rp.packed_to_dict(good), 30)):
        write_npz(tmp_path / "replays" / name, data)
        index.add(tmp_path / "replays" / name, rows, "selfplay")
    with dr.DeviceReplay.from_store(tmp_path, device="host") as store:
        assert store.skipped == ["b.npz"]
        i = store.info()
        assert (i["rows"], i["segments"], i["raw_rows"]) == (70, 2, 0)
        rows, kinds = [0, 39, 40, 69], [0, 1, 2, 1]
        assert not same(store.batch(rows, kinds), reference((s, pi, z, mask), rows, kinds))
    with dr.DeviceReplay.from_store(tmp_path, device="host", window_rows=30) as store:
        assert store.resident_ids().tolist() == list(range(40, 70))
    with dr.DeviceReplay.from_store(tmp_path, sources=("stockfish",), device="host") as store:
        assert store.info()["rows"] == 0 and store.skipped == []
    assert dr.main(["info", str(tmp_path)]) == 0
    import json
    report = json.loads(capsys.readouterr().out)
    assert report["rows"] == 70 and report["segments"] == 2 and report["skipped"] == ["b.npz"] and report["raw_rows"] == 0
    assert report["dense_bytes"] == 70 * rp.DENSE_ROW_BYTES and 0 < report["packed_bytes"] < report["dense_bytes"] // 50
