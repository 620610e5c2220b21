"""Packed training rows on the device (include/m0_rowpack.h): the pack and unpack kernels through m0_rowpack_pack / _unpack
against the host calls (which tests/test_rowpack.py compares with the numpy restatement), the round trip, M0Backend.score of
packed rows against the dense rows, score_shards over a packed copy of a store, and import_pgn(packed=True).  Every comparison
is of bit patterns; nothing here has a tolerance."""
import itertools
import os

import numpy as np
import pytest

from matrix0_amd import rowpack as rp
from tests import net_layer_cases as net_cases
from tests import rowpack_cases as rc

pytestmark = pytest.mark.gpu

BATCHES = (1, 3, 65, 257, 2051)        # four rows per workgroup: a partial one, whole ones and a partial last one
SMALL = dict(planes=19, channels=64, blocks=2, attention_heads=4, policy_size=4672, norm="group", activation="silu", preact=True,
             policy_factor_rank=32, self_supervised=False)


def _dense_equal(got, want):
    return all(rc.same_bits(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("with_mask", (True, False), ids=("mask", "nomask"))
@pytest.mark.parametrize("B", BATCHES)
def test_kernels_equal_the_host_calls_and_round_trip(B, with_mask):
    s, pi, z, mask, kinds = rc.edge_rows(B, seed=B, with_mask=with_mask)
    host = _host_pack(s, pi, z, mask)
    dev = rp.pack_rows(s, pi, z, mask, device=0)
    assert rc.same_packed(dev, host) is None, rc.same_packed(dev, host)
    want_rows, want_masks = rc.expected_kinds(kinds, with_mask)
    assert np.array_equal(dev.fields["row_kind"], want_rows) and np.array_equal(dev.fields["mask_kind"], want_masks)
    # m0_rowpack_unpack(m0_rowpack_pack(x)) == x, and the device's dense rows are the host's
    got = rp.unpack_rows(dev, device=0)
    assert _dense_equal(got, (s, pi, z, mask))
    # the same rows at other row indices and in another batch: a row's bytes depend on the row alone
    shift = 3 % B
    order = np.roll(np.arange(B), shift)
    rolled = rp.pack_rows(s[order], pi[order], z[order], None if mask is None else mask[order], device=0)
    for i in (0, B // 2, B - 1):
        j = int(np.flatnonzero(order == i)[0])
        assert rc.same_packed(rolled.rows(j, j + 1), dev.rows(i, i + 1)) is None, (i, j)
    assert rc.same_packed(rp.pack_rows(s, pi, z, mask, device=0), dev) is None          # and a repetition


def _host_pack(s, pi, z, mask):
    """pack_rows through m0_rowpack_pack_host whatever devices there are"""
    import ctypes as C
    from matrix0_amd import _lib
    n = len(s)
    sizes = np.zeros(3, np.int64)
    empty = rp.PackedRows(np.zeros((n, rp.POS_BYTES), np.uint8), np.empty(n, np.float32), np.empty(n + 1, np.int64),
                          np.empty(0, np.uint16), np.empty(0, np.float32), np.empty(n + 1, np.int64), np.empty(0, np.uint16),
                          np.empty((0, 19, 8, 8), np.float32), np.empty((0, 4672), np.float32), None)
    a = empty.c_arrays()
    args = [_lib.ptr(np.ascontiguousarray(x)) if x is not None else None for x in (s, pi, z, mask)]
    assert _lib.lib().m0_rowpack_pack_host(*args, n, C.byref(a), _lib.ptr(sizes)) == _lib.M0_ERR_INVALID      # sizes first
    npi, nmk, raw = (int(x) for x in sizes)
    out = rp.PackedRows(empty.pos, empty.z, empty.pi_off, np.empty(npi, np.uint16), np.empty(npi, np.float32), empty.mask_off,
                        np.empty(nmk, np.uint16), np.empty((raw, 19, 8, 8), np.float32), np.empty((raw, 4672), np.float32),
                        None if mask is None else np.empty((raw, 4672), np.uint8))
    a = out.c_arrays()
    assert _lib.lib().m0_rowpack_pack_host(*args, n, C.byref(a), _lib.ptr(sizes)) == _lib.M0_OK, _lib.last_error()
    return out


def test_the_worker_rows_round_trip_on_the_device():
    s, pi, z, mask = rc.worker_rows()
    dev = rp.pack_rows(s, pi, z, mask, device=0)
    assert rc.same_packed(dev, _host_pack(s, pi, z, mask)) is None
    assert dev.kinds() == {"rows": {"packed": 375, "raw": 0}, "masks": {"none": 0, "legal": 375, "list": 0}}
    assert _dense_equal(rp.unpack_rows(dev, device=0), (s, pi, z, mask))


def test_too_small_a_capacity_returns_the_sizes_and_writes_nothing():
    import ctypes as C
    from matrix0_amd import _lib
    s, pi, z, mask, _ = rc.edge_rows(65, seed=65)
    n = len(s)
    sizes = np.zeros(3, np.int64)
    out = rp.PackedRows(np.full((n, rp.POS_BYTES), 0xAB, np.uint8), np.full(n, -7, np.float32), np.full(n + 1, -7, np.int64),
                        np.full(8, 0xABAB, np.uint16), np.full(8, -7, np.float32), np.full(n + 1, -7, np.int64),
                        np.full(8, 0xABAB, np.uint16), np.full((1, 19, 8, 8), -7, np.float32), np.full((1, 4672), -7, np.float32),
                        np.full((1, 4672), 0xAB, np.uint8))
    a = out.c_arrays()
    rcode = _lib.lib().m0_rowpack_pack(0, _lib.ptr(s), _lib.ptr(pi), _lib.ptr(z), _lib.ptr(mask), n, C.byref(a), _lib.ptr(sizes))
    assert rcode == _lib.M0_ERR_INVALID
    want = _host_pack(s, pi, z, mask)
    assert sizes.tolist() == [len(want.pi_idx), len(want.mask_idx), len(want.raw_planes)] and sizes[0] > 8 and sizes[2] > 1
    assert (out.pos == 0xAB).all() and (out.z == -7).all() and (out.pi_off == -7).all() and (out.pi_idx == 0xABAB).all()
    assert (out.raw_planes == -7).all() and (out.raw_mask == 0xAB).all() and (out.mask_off == -7).all()


@pytest.fixture(scope="module")
def small_net():
    from matrix0_amd.backend import M0Backend
    be = M0Backend.from_state_dict(SMALL, net_cases.weights(SMALL, sharp=True))
    yield be
    be.close()


@pytest.mark.parametrize("B", (5, 65))
def test_score_of_packed_rows_equals_score_of_the_dense_rows(small_net, B):
    s, pi, z, mask, kinds = rc.edge_rows(B, seed=0)
    packed = rp.pack_rows(s, pi, z, mask, device=0)
    k = packed.kinds()
    assert k["rows"]["raw"] >= 1 and k["masks"]["list"] >= 2 and k["masks"]["legal"] >= 1
    bare = rp.pack_rows(s, pi, z, None, device=0)
    for mode, loss, smooth in itertools.product(("legal", "target", "none"), ("mse", "huber"), (0.0, 0.05)):
        opts = dict(mask_mode=mode, value_loss=loss, label_smoothing=smooth, huber_delta=0.7)
        want = small_net.score(s, pi, z, mask, **opts)
        got = small_net.score(packed=packed, **opts)
        assert rc.same_bits(got, want), (mode, loss, smooth, np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1)))
        if mode != "legal":
            assert rc.same_bits(small_net.score(packed=bare, **opts), small_net.score(s, pi, z, None, **opts)), (mode, loss, smooth)
    with pytest.raises(ValueError):
        small_net.score(packed=bare, mask_mode="legal")
    assert rc.same_bits(small_net.score(packed=packed), small_net.score(s, pi, z, mask))          # the mode resolved
    assert rc.same_bits(small_net.score(packed=bare), small_net.score(s, pi, z, None))


def _store(base, shards):
    from matrix0_amd.data_writer import ShardIndex, write_npz
    os.makedirs(base / "replays", exist_ok=True)
    index = ShardIndex(base)
    for name, data in shards.items():
        write_npz(base / "replays" / name, data)
        index.add(base / "replays" / name, len(data["s"]), "selfplay")


def test_score_shards_over_a_packed_copy_equals_the_dense_store(small_net, tmp_path):
    from matrix0_amd import score as sc
    s, pi, z, mask = rc.worker_rows()
    es, epi, ez, emask, _ = rc.edge_rows(32, seed=0)
    finite = np.isfinite(epi).all(axis=1) & (emask <= 1).all(axis=1)
    shards = {"a.npz": dict(s=s[:40], pi=pi[:40], z=z[:40], legal_mask=mask[:40], meta_moves=np.array([40])),
              "b.npz": dict(s=s[40:70], pi=pi[40:70], z=z[40:70].reshape(-1, 1)),
              "c.npz": dict(s=es[finite], pi=epi[finite], z=ez[finite], legal_mask=emask[finite])}
    _store(tmp_path / "dense", shards)
    assert rp.main(["pack", str(tmp_path / "dense"), str(tmp_path / "packed"), "--device", "0"]) == 0
    for opts in (dict(), dict(label_smoothing=0.05, value_loss="huber"), dict(mask_mode="target")):
        dense = sc.score_shards(tmp_path / "dense", small_net, batch=16, **opts)
        packed = sc.score_shards(tmp_path / "packed", small_net, batch=16, **opts)
        assert not dense["skipped"] and dense["rows"] == 70 + int(finite.sum())
        assert packed == dense


def test_import_pgn_packed_unpacks_to_the_dense_import(tmp_path):
    from matrix0_amd import arena, game_import as gi
    from tests import replay_util as ru
    games = ru.fixture_games()[::13][:10]
    paths = [arena.save_pgn(ru.shim_replay(None, toks)["moves"], result, {"Round": i + 1}, str(tmp_path / "pgn"), i)
             for i, (toks, result) in enumerate(games)]
    pgn = tmp_path / "ten.pgn"
    pgn.write_text("\n".join(open(p).read() for p in paths))
    for more in (dict(), dict(legal_mask=False), dict(ssl_tasks=("piece", "control"))):
        tag = "_".join(more) or "plain"
        dense = gi.import_pgn(str(pgn), str(tmp_path / ("dense_" + tag)), shard_size=256, **more)
        packed = gi.import_pgn(str(pgn), str(tmp_path / ("packed_" + tag)), shard_size=256, packed=True, **more)
        assert packed == dense and dense["games_kept"] == 10 and dense["shards"] >= 2
        for name in sorted(os.listdir(tmp_path / ("dense_" + tag))):
            want = dict(np.load(tmp_path / ("dense_" + tag) / name))
            with np.load(tmp_path / ("packed_" + tag) / name) as d:
                assert "rowpack_version" in d.files and "pi" not in d.files
            kinds = rp.read_shard(tmp_path / ("packed_" + tag) / name)[0].kinds()
            assert kinds["rows"]["raw"] == 0 and kinds["masks"]["list"] == 0                     # imported rows always pack
            for device in ("host", 0):
                got = rp.load_shard(tmp_path / ("packed_" + tag) / name, device=device)
                assert set(got) == set(want), (tag, name)
                for k in want:
                    assert rc.same_bits(got[k], want[k]), (tag, name, k, device)


def test_score_shards_lists_a_packed_shard_that_does_not_hold_together_as_skipped(small_net, tmp_path):
    from matrix0_amd import score as sc
    from matrix0_amd.data_writer import ShardIndex
    s, pi, z, mask = (a[:24] for a in rc.worker_rows())
    _store(tmp_path / "store", {"a.npz": dict(s=s, pi=pi, z=z, legal_mask=mask)})
    good = rp.pack_rows(s, pi, z, mask, device=0)
    bad_columns = rp.packed_to_dict(good)
    bad_columns["rowpack_pi_idx"] = bad_columns["rowpack_pi_idx"][::-1].copy()             # columns that do not ascend
    short = rp.packed_to_dict(good)
    short["rowpack_z"] = short["rowpack_z"][:5]                                            # a truncated key
    index = ShardIndex(tmp_path / "store")
    for name, d in (("b.npz", bad_columns), ("c.npz", short), ("d.npz", rp.packed_to_dict(good))):
        rp.write_npz(tmp_path / "store" / "replays" / name, d)
        index.add(tmp_path / "store" / "replays" / name, 24, "selfplay")
    r = sc.score_shards(tmp_path / "store", small_net, batch=16)
    assert r["skipped"] == ["b.npz", "c.npz"] and list(r["by_shard"]) == ["a.npz", "d.npz"] and r["rows"] == 48
    assert r["by_shard"]["a.npz"] == r["by_shard"]["d.npz"]
