"""The SSL target maps of a batch on the CPU (include/m0_batch_ssl.h, matrix0_amd/device_replay.py; no GPU): the host call
m0_rowstore_batch_ssl_host and a host store.  The maps must be those of the planes the same call writes -- against
oracle/ssl_ref.py, which tests/golden/ssl_targets.npz pins to the reference and which never sees the code under test -- the other
four arrays must stay those of m0_rowstore_batch_host, and a refusal must leave all six outputs alone.  Every comparison is of bit
patterns; nothing here has a tolerance."""
import ctypes as C
import functools

import numpy as np
import pytest

from matrix0_amd import _lib, device_replay as dr, rowpack as rp
from oracle import ssl_ref
from tests import rowpack_cases as rc
from tests import ssl_score_cases as sc
from tests.test_device_replay import batch_host, canaries, same, untouched

BATCHES = (1, 3, 5, 65, 257)
ORDER = ("threat", "pin", "fork", "control")


def batch_ssl_host(packed, rows, kinds):
    """(s, pi, z, mask or None, ssl f32 [B,17,8,8], ssl_status i32 [B]) of m0_rowstore_batch_ssl_host"""
    rows = np.ascontiguousarray(rows, np.int64)
    kinds = None if kinds is None else np.ascontiguousarray(kinds, np.uint8)
    B = len(rows)
    s, pi, z = np.empty((B, 19, 8, 8), np.float32), np.empty((B, 4672), np.float32), np.empty(B, np.float32)
    mask = np.empty((B, 4672), np.uint8) if packed.has_mask else None
    ssl, status = np.empty((B, 17, 8, 8), np.float32), np.empty(B, np.int32)
    a = packed.c_arrays()
    p = _lib.ptr
    rcode = _lib.lib().m0_rowstore_batch_ssl_host(C.byref(a), p(rows), p(kinds), B, p(s), p(pi), p(z), p(mask), p(ssl), p(status))
    assert rcode == _lib.M0_OK, _lib.last_error()
    return s, pi, z, mask, ssl, status


def oracle_maps(planes):
    """oracle.ssl_ref.targets of planes [n,19,8,8], laid out as the batch lays them out: f32 [n,17,8,8]"""
    out = np.empty((len(planes), 17, 8, 8), np.float32)
    for b, row in enumerate(planes):
        t = ssl_ref.targets(row)
        out[b, :13] = t["piece"]
        for k, name in enumerate(ORDER):
            out[b, 13 + k] = t[name]
    return out


def canaries6(B, with_mask=True):
    out = canaries(B, with_mask)
    return out + [np.full((B, 17, 8, 8), -7, np.float32), np.full(B, -7, np.int32)]


def raw_batch_ssl(store, rows, kinds, out, with_mask=True):
    """m0_rowstore_batch_ssl on `out` = the four (or three) arrays, then ssl and ssl_status; a None entry is a null pointer"""
    rows = np.ascontiguousarray(rows, np.int64)
    kinds = None if kinds is None else np.ascontiguousarray(kinds, np.uint8)
    ptrs = [_lib.ptr(a) for a in out]
    if not with_mask:
        ptrs.insert(3, None)
    return _lib.lib().m0_rowstore_batch_ssl(store._h, _lib.ptr(rows), _lib.ptr(kinds), len(rows), *ptrs, 0, None)


@functools.lru_cache(maxsize=None)
def edge(B, with_mask):
    s, pi, z, mask, kinds = rc.edge_rows(B, seed=B, with_mask=with_mask)
    return rp.pack_rows(s, pi, z, mask, device="host"), kinds


@functools.lru_cache(maxsize=None)
def worker_case():
    """Every fifth worker row under each of the three kinds, 225 rows, all PACKED: (packed, rows, kinds, the host call's six
    arrays, the oracle's maps of the planes it wrote)"""
    s, pi, z, mask = (a[::5] for a in rc.worker_rows())
    packed = rp.pack_rows(s, pi, z, mask, device="host")
    assert packed.n == 75 and packed.kinds()["rows"]["raw"] == 0
    rows, kinds = np.tile(np.arange(75), 3), np.repeat([0, 1, 2], 75)
    got = batch_ssl_host(packed, rows, kinds)
    return packed, rows, kinds, got, oracle_maps(got[0])


@pytest.mark.parametrize("with_mask", (True, False), ids=("mask", "nomask"))
@pytest.mark.parametrize("B", BATCHES)
def test_the_four_arrays_are_those_of_the_call_without_maps(B, with_mask):
    packed, _ = edge(B, with_mask)
    rows, kinds = np.arange(B), np.arange(B) % 3
    got = batch_ssl_host(packed, rows, kinds)
    assert not same(got[:4], batch_host(packed, rows, kinds))
    assert got[4].shape == (B, 17, 8, 8) and got[5].shape == (B,) and set(got[5].tolist()) <= {0, 1}


def test_the_maps_of_packed_rows_equal_the_independent_oracle():
    _, rows, kinds, got, want = worker_case()
    assert len(rows) == 225
    assert not got[5].any()
    differ = np.flatnonzero((got[4].view(np.uint32) != want.view(np.uint32)).any(axis=(1, 2, 3)))
    assert differ.size == 0, [(int(rows[b]), int(kinds[b])) for b in differ[:8]]
    # the maps say something: threats, forks and both signs of control occur
    assert got[4][:, 13].any() and got[4][:, 15].any() and (got[4][:, 16] > 0).any() and (got[4][:, 16] < 0).any()
    assert not got[4][:, 14].any()                                           # the reference's pin map is identically zero


def test_usable_and_unusable_raw_rows():
    # the edge rows, in a store's worth of arrays with masks
    packed, edge_kinds = edge(257, True)
    counts = np.bincount(edge_kinds, minlength=16)
    assert set(counts.tolist()) == {16, 17}
    raw = packed.fields["row_kind"] == rc.RAW
    assert raw[np.isin(edge_kinds, (3, 4, 15))].all() and raw.sum() == counts[[3, 4, 15]].sum()
    rows, kinds = np.arange(257), np.arange(257) % 3
    got = batch_ssl_host(packed, rows, kinds)
    assert sorted(np.flatnonzero(got[5] == 1).tolist()) == np.flatnonzero(edge_kinds == 4).tolist()
    assert set(got[5].tolist()) == {0, 1}
    assert not got[4][got[5] == 1].view(np.uint32).any()                     # all 17 maps written as +0
    ok = got[5] == 0
    assert rc.same_bits(got[4][ok], oracle_maps(got[0][ok]))
    assert {int(k) for k in kinds[edge_kinds == 3]} == {int(k) for k in kinds[edge_kinds == 15]} == {0, 1, 2}
    # eight rows of planes that are no positions, without masks, under every kind
    names, _, planes = sc._rows(100, 19)
    take = [n for n in names if n.startswith("unusable: ")] + ["empty board", "every square occupied", "random board 0", "random board 1"]
    assert len(take) == 8 and sum(n.startswith("unusable: ") for n in take) == 4
    s = np.stack([planes[names.index(n)] for n in take]).astype(np.float32)
    rng = np.random.default_rng(8)
    pi = np.stack([rc.seeded_pi(rng, 5) for _ in take])
    hand = rp.pack_rows(s, pi, np.linspace(-1, 1, 8).astype(np.float32), None, device="host")
    assert (hand.fields["row_kind"][:4] == rc.RAW).all()
    rows, kinds = np.tile(np.arange(8), 3), np.repeat([0, 1, 2], 8)
    got = batch_ssl_host(hand, rows, kinds)
    assert got[3] is None and rc.same_bits(got[0][:8], s)
    assert np.flatnonzero(got[5] == 1).tolist() == np.flatnonzero(rows < 4).tolist() and set(got[5].tolist()) == {0, 1}
    assert not got[4][got[5] == 1].view(np.uint32).any()
    ok = got[5] == 0
    assert ok.sum() == 12 and rc.same_bits(got[4][ok], oracle_maps(got[0][ok]))


def test_the_maps_are_those_of_the_output_planes_not_moved_maps_of_the_stored_row():
    _, rows, kinds, got, _ = worker_case()
    ssl = got[4]
    none, hflip, rot180 = ssl[kinds == 0], ssl[kinds == 1], ssl[kinds == 2]
    assert rc.same_bits(hflip, none[..., ::-1])                              # mirrored in the columns, every row
    moved = none[..., ::-1, ::-1]
    differ = (rot180.view(np.uint32) != np.ascontiguousarray(moved).view(np.uint32)).any(axis=(1, 2, 3))
    assert differ.any()                                                      # pawn attacks point one way in tensor space
    assert rc.same_bits(rot180[:, :13], moved[:, :13])                       # the pieces themselves do move with the board
    assert differ.sum() == 57                                                # of these 75 rows


def test_a_refused_call_leaves_all_six_outputs_untouched():
    packed, _ = edge(65, True)
    bare = rp.pack_rows(*rc.edge_rows(24, seed=1)[:3], None, device="host")
    with dr.DeviceReplay("host") as store, dr.DeviceReplay("host", with_mask=False) as nomask:
        store.append(packed)
        nomask.append(bare)
        out = canaries6(3)
        assert raw_batch_ssl(store, [1, 65, 2], None, out) == _lib.M0_ERR_INVALID and "65" in _lib.last_error() and untouched(out)
        assert raw_batch_ssl(store, [1, 2, 3], [0, 3, 0], out) == _lib.M0_ERR_INVALID and untouched(out)
        assert raw_batch_ssl(store, [1, 2, 3], None, out[:4] + [None, out[5]]) == _lib.M0_ERR_INVALID and untouched(out)
        assert "null" in _lib.last_error()
        assert raw_batch_ssl(store, [1, 2, 3], None, out[:5] + [None]) == _lib.M0_ERR_INVALID and untouched(out)
        assert raw_batch_ssl(store, [], None, out) == _lib.M0_ERR_INVALID and untouched(out)
        assert raw_batch_ssl(store, [1, 2, 3], None, out[:3] + out[4:], with_mask=False) == _lib.M0_ERR_INVALID and untouched(out)
        assert raw_batch_ssl(nomask, [1, 2, 3], None, out) == _lib.M0_ERR_INVALID and untouched(out)          # a superfluous mask
        # device outputs of a host store
        ptrs = [_lib.ptr(a) for a in out]
        rows3 = np.array([1, 2, 3], np.int64)
        assert _lib.lib().m0_rowstore_batch_ssl(store._h, _lib.ptr(rows3), None, 3, *ptrs, 1, None) == _lib.M0_ERR_INVALID
        assert untouched(out)
        # and the same calls are fine once nothing is wrong with them
        assert raw_batch_ssl(store, [1, 2, 3], [0, 2, 0], out) == _lib.M0_OK and not untouched(out[4:5]) and not untouched(out[5:])
        want = batch_ssl_host(packed, [1, 2, 3], [0, 2, 0])
        assert not same(out, want)
    # the host call over one set of arrays refuses in the same way
    out = canaries6(3)
    a = packed.c_arrays()
    p = _lib.ptr
    host = lambda rows, kinds, o: _lib.lib().m0_rowstore_batch_ssl_host(
        C.byref(a), p(np.asarray(rows, np.int64)), p(None if kinds is None else np.asarray(kinds, np.uint8)), len(rows), *[p(x) for x in o])
    assert host([1, 65, 2], None, out) == _lib.M0_ERR_INVALID and "65" in _lib.last_error() and untouched(out)
    assert host([1, 2, 3], [0, 3, 0], out) == _lib.M0_ERR_INVALID and untouched(out)
    assert host([1, 2, 3], None, out[:4] + [None, out[5]]) == _lib.M0_ERR_INVALID and untouched(out)
    assert host([1, 2, 3], None, out[:5] + [None]) == _lib.M0_ERR_INVALID and untouched(out)
    assert host([1, 2, 3], None, out[:3] + [None] + out[4:]) == _lib.M0_ERR_INVALID and untouched(out)          # a missing mask


def test_a_host_store_gives_what_the_host_call_gives():
    packed, _ = edge(65, True)
    rows, kinds = np.arange(65)[::-1].copy(), np.arange(65) % 3
    want = batch_ssl_host(packed, rows, kinds)
    assert want[5].any() and not want[5].all()
    with dr.DeviceReplay("host") as store:
        store.append(packed.rows(0, 30))
        store.append(packed.rows(30, 65))
        got = store.batch(rows, kinds, ssl=True)
        assert len(got) == 6 and got[4].dtype == np.float32 and got[5].dtype == np.int32
        assert not same(got, want)
        assert not same(store.batch(rows, 2, ssl=True), batch_ssl_host(packed, rows, np.full(65, 2)))
        n = 0
        for s, pi, z, mask, ssl, status, ids, kind in store.batches(16, epochs=1, seed=4, ssl=True):
            assert ssl.shape == (16, 17, 8, 8) and status.shape == (16,) and ids.shape == (16,) and kind in (0, 1, 2)
            assert not same((s, pi, z, mask, ssl, status), batch_ssl_host(packed, ids, np.full(16, kind)))
            n += 1
        assert n == 4
        t = dr.ssl_targets(got[4])
        assert list(t) == ["piece", "threat", "pin", "fork", "control"]
        assert t["piece"].shape == (65, 13, 8, 8) and all(t[k].shape == (65, 8, 8) for k in ORDER)
        assert all(np.shares_memory(v, got[4]) for v in t.values())
        assert rc.same_bits(t["piece"], got[4][:, :13]) and all(rc.same_bits(t[k], got[4][:, 13 + i]) for i, k in enumerate(ORDER))
        with pytest.raises(ValueError):
            dr.ssl_targets(got[0])
    bare = rp.pack_rows(*rc.edge_rows(24, seed=1)[:3], None, device="host")
    with dr.DeviceReplay("host", with_mask=False) as store:
        store.append(bare)
        got = store.batch([0, 23, 4], [1, 2, 0], ssl=True)
        assert len(got) == 5 and not same(got, [w for w in batch_ssl_host(bare, [0, 23, 4], [1, 2, 0]) if w is not None])
        assert len(next(store.batches(8, epochs=1, ssl=True))) == 7


def test_without_ssl_every_call_returns_what_it_returned():
    packed, _ = edge(65, True)
    with dr.DeviceReplay("host") as store:
        store.append(packed)
        got = store.batch([3, 4], [1, 2])
        assert len(got) == 4 and len(store.batch([3, 4], [1, 2], ssl=False)) == 4
        assert not same(got, batch_host(packed, [3, 4], [1, 2]))
        assert len(next(store.batches(16, epochs=1))) == 6 and len(next(store.batches(16, epochs=1, ssl=False))) == 6
    bare = rp.pack_rows(*rc.edge_rows(24, seed=1)[:3], None, device="host")
    with dr.DeviceReplay("host", with_mask=False) as store:
        store.append(bare)
        assert len(store.batch([0, 1])) == 3 and len(next(store.batches(8, epochs=1))) == 5
