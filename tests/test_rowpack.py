"""Packed training rows on the CPU (include/m0_rowpack.h): m0_rowpack_pack_host / m0_rowpack_unpack_host against the numpy
restatement tests/rowpack_ref.py (which shares no code with the engine) on the golden rows and on every edge of the format,
the kernels' lane split as a loop against the straight loops, the reference's mutations, the sanitizer build, and the files:
pack and unpack of a store, the reader over mixed stores, the shard table.  Every comparison is of bit patterns."""
import hashlib
import os
import sqlite3
import subprocess

import numpy as np
import pytest

from matrix0_amd import rowpack as rp
from tests import planes_cases as pc
from tests import rowpack_cases as rc
from tests import rowpack_ref as ref
from tests import rowpack_shim as shim
from tests.golden_ref import load_npz

HERE = os.path.dirname(os.path.abspath(__file__))


def host_pack(s, pi, z, mask=None):
    return rp.pack_rows(s, pi, z, mask, device="host")


def host_unpack(packed):
    return rp.unpack_rows(packed, device="host")


def differs_from_ref(packed, want):
    """The first array of a PackedRows that is not the reference's, or None"""
    for k in ("pos", "pi_off", "pi_idx", "pi_val", "mask_off", "mask_idx", "raw_planes", "raw_pi", "raw_mask"):
        if not rc.same_bits(getattr(packed, k), want[k]):
            return k
    return None


def check_against_ref(s, pi, z, mask):
    """Host pack == reference pack, host unpack == source, lane split == straight loops; returns the PackedRows"""
    packed = host_pack(s, pi, z, mask)
    want = ref.pack_rows(s, pi, mask)
    assert differs_from_ref(packed, want) is None, differs_from_ref(packed, want)
    assert rc.same_bits(packed.z, np.asarray(z, np.float32))
    got = host_unpack(packed)
    assert all(rc.same_bits(g, w) for g, w in zip(got, (s, pi, z, mask)))
    assert rc.same_packed(shim.pack_lanes(s, pi, z, mask), packed) is None
    assert all(rc.same_bits(g, w) for g, w in zip(shim.unpack_lanes(packed), got))
    return packed, want


# ---- golden rows ------------------------------------------------------------------------------------------------------------------
def test_the_worker_rows_pack_as_the_reference_packs_them_and_come_back():
    s, pi, z, mask = rc.worker_rows()
    packed, want = check_against_ref(s, pi, z, mask)
    assert packed.kinds() == {"rows": {"packed": 375, "raw": 0}, "masks": {"none": 0, "legal": 375, "list": 0}}
    counts = np.diff(packed.pi_off)
    assert counts.min() == 1 and counts.max() == 45
    # the reference's own way back (oracle FEN -> encode_board, legal columns) gives the source too
    for i in range(0, 375, 7):
        planes, pi_i, mask_i = ref.unpack_row(want["rows"][i], True)
        assert rc.same_bits(planes, s[i]) and rc.same_bits(pi_i, pi[i]) and rc.same_bits(mask_i, mask[i]), i
    assert packed.nbytes < 375 * 400 and rp.DENSE_ROW_BYTES == 28228


@pytest.fixture(scope="module")
def encoding_rows():
    """The 10 016 golden encodings as rows: planes as tests/test_planes_decode.py builds them, the mask from the legal indices, pi
    seeded visit fractions over them"""
    g = load_npz("ref_encoding.npz")
    n = len(g["fens"])
    nlegal = g["nlegal"].astype(np.int64)
    planes = np.zeros((n, 19, 8, 8), np.float32)
    planes[:, :17] = np.unpackbits(g["plane_bits"], axis=2).reshape(n, 17, 8, 8)
    planes[:, 17] = g["counters"][:, 0, None, None]
    planes[:, 18] = g["counters"][:, 1, None, None]
    rows, cols = np.repeat(np.arange(n), nlegal), g["idx"].astype(np.int64)
    mask = np.zeros((n, 4672), np.uint8)
    mask[rows, cols] = 1
    rng = np.random.default_rng(20)
    visits = rng.integers(0, 40, size=len(cols)).astype(np.float64)            # some legal moves get no visit
    total = np.maximum(np.bincount(rows, visits, minlength=n), 1.0)
    pi = np.zeros((n, 4672), np.float32)
    pi[rows, cols] = (visits / total[rows]).astype(np.float32)
    z = rng.integers(-1, 2, size=n).astype(np.float32)
    return planes, pi, z, mask, [str(f) for f in g["fens"]]


def test_every_golden_encoding_is_packed_with_a_legal_mask_and_comes_back(encoding_rows):
    s, pi, z, mask, fens = encoding_rows
    assert len(s) == 10016
    packed = host_pack(s, pi, z, mask)
    k = packed.kinds()
    assert k["rows"]["raw"] == 0 and k["masks"] == {"none": 0, "legal": 10016, "list": 0}, k        # the share of RAW rows is 0
    assert all(rc.same_bits(g, w) for g, w in zip(host_unpack(packed), (s, pi, z, mask)))
    # against the reference on every row; the stored positions are the golden FENs (counters capped) on every 16th row and on
    # every row with en passant, castling rights or a saturated counter
    want = ref.pack_rows(s, pi, mask)
    assert differs_from_ref(packed, want) is None, differs_from_ref(packed, want)
    f = packed.fields
    sel = np.unique(np.concatenate([np.arange(0, 10016, 16), np.flatnonzero(f["ep"] != 255), np.flatnonzero(f["halfmove"] == 99),
                                    np.flatnonzero(f["fullmove"] == 199), np.flatnonzero(f["castling"] != 0)[::8]]))
    assert (f["ep"] != 255).sum() == 3 and (f["halfmove"] == 99).sum() >= 1 and (f["fullmove"] == 199).sum() >= 1
    for i in sel:
        got, gold = ref.fen_of(packed.pos[i]).split(), fens[i].split()
        assert got[:4] == gold[:4] and got[4:] == [str(min(int(gold[4]), 99)), str(min(int(gold[5]), 199))], fens[i]


# ---- edges ------------------------------------------------------------------------------------------------------------------------
def test_en_passant_squares_are_stored_with_a_mask_and_unknown_without():
    s, pi, z, mask, eps = rc.ep_rows()
    assert len(s) == 13
    packed, _ = check_against_ref(s, pi, z, mask)
    squares = [255 if e is None else (ord(e[0]) - 97) + 8 * (int(e[1]) - 1) for e in eps]
    assert packed.fields["ep"].tolist() == squares and sum(e is not None for e in eps) == 7
    assert packed.kinds()["masks"]["legal"] == 13 and packed.kinds()["rows"]["packed"] == 13
    bare, _ = check_against_ref(s, pi, z, None)
    assert (bare.fields["ep"] == 255).all() and bare.kinds()["masks"]["none"] == 13 and not bare.has_mask


def test_every_malformed_row_is_raw_and_exact():
    rows = pc.malformed_rows()
    s = np.stack([r[2] for r in rows])
    mask = np.stack([r[3] for r in rows])
    pi = ((mask > 0) / np.maximum((mask > 0).sum(axis=1, keepdims=True), 1)).astype(np.float32)
    z = np.zeros(len(rows), np.float32)
    for m in (mask, None):
        packed, _ = check_against_ref(s, pi, z, m)
        for (name, status, _, _), kind, mk in zip(rows, packed.fields["row_kind"], packed.fields["mask_kind"]):
            mismatch = status == pc.MASK_MISMATCH
            assert kind == (rc.PACKED if mismatch else rc.RAW), name
            assert mk == (rc.MASK_NONE if m is None else rc.MASK_LIST if m is not None and (mismatch or kind == rc.RAW) else rc.MASK_LEGAL), name
        assert len(packed.raw_planes) == sum(r[1] != pc.MASK_MISMATCH for r in rows)


@pytest.mark.parametrize("with_mask", (True, False), ids=("mask", "nomask"))
def test_row_kinds_mask_kinds_and_entry_counts(with_mask):
    s, pi, z, mask, kinds = rc.edge_rows(4 * rc.EDGES + 1, seed=7, with_mask=with_mask)
    packed, _ = check_against_ref(s, pi, z, mask)
    rows, masks = rc.expected_kinds(kinds, with_mask)
    assert np.array_equal(packed.fields["row_kind"], rows) and np.array_equal(packed.fields["mask_kind"], masks)
    counts = np.diff(packed.pi_off)
    for k, want in zip(range(5, 12), rc.ENTRY_COUNTS):
        assert (counts[kinds == k] == want).all(), (k, want)
    assert (counts[kinds == 12] == 4).all() and (counts[kinds == 13] == 16).all() and (counts[kinds == 14] == 4).all()
    i = int(np.flatnonzero(kinds == 12)[0])
    assert packed.pi_idx[packed.pi_off[i]:packed.pi_off[i + 1]].tolist() == [0, 63, 64, 4671]
    i = int(np.flatnonzero(kinds == 14)[0])
    assert sorted(packed.pi_val[packed.pi_off[i]:packed.pi_off[i + 1]].view(np.uint32).tolist()) == sorted(rc.ODD_BITS.tolist())
    if with_mask:                                        # a LIST mask is exactly the edited mask
        i = int(np.flatnonzero(kinds == 2)[0])
        assert packed.mask_idx[packed.mask_off[i]:packed.mask_off[i + 1]].tolist() == np.flatnonzero(mask[i]).tolist()


def test_a_row_packs_to_the_same_bytes_wherever_it_stands():
    s, pi, z, mask, _ = rc.edge_rows(37, seed=3)
    whole = host_pack(s, pi, z, mask)
    order = np.roll(np.arange(37), 5)
    rolled = host_pack(s[order], pi[order], z[order], mask[order])
    for j, i in enumerate(order):
        assert rc.same_packed(rolled.rows(j, j + 1), whole.rows(i, i + 1)) is None, i
        assert rc.same_packed(host_pack(s[i:i + 1], pi[i:i + 1], z[i:i + 1], mask[i:i + 1]), whole.rows(i, i + 1)) is None, i


def test_each_mutation_of_the_reference_fails_some_row():
    ws, wpi, wz, wm = rc.worker_rows()
    es, epi, ez, em, eps = rc.ep_rows()
    ms, mpi, mz, mm, kinds = rc.edge_rows(2 * rc.EDGES, seed=1)
    castle_s, castle_m = pc.encode("r3k2r/8/8/8/8/8/8/R3K2R w Kq - 0 1")
    sets = {"entry_by_value": (ms, mpi, mm), "drop_ep": (es, epi, em), "legal_on_mismatch": (ms, mpi, mm),
            "castling_from_men": (castle_s[None], (castle_m / castle_m.sum()).astype(np.float32)[None], castle_m[None])}
    for name, (s, pi, mask) in sets.items():
        packed = host_pack(s, pi, np.zeros(len(s), np.float32), mask)
        assert differs_from_ref(packed, ref.pack_rows(s, pi, mask)) is None, name
        mutated = ref.pack_rows(s, pi, mask, ref.Mutations(**{name: True}))
        assert differs_from_ref(packed, mutated) is not None, name
    assert host_pack(castle_s[None], wpi[:1], wz[:1], castle_m[None]).fields["castling"][0] == 1 | 8


def test_arrays_that_do_not_hold_together_are_refused():
    s, pi, z, mask, _ = rc.edge_rows(20, seed=0)
    good = host_pack(s, pi, z, mask)

    def broken(**change):
        p = rp.PackedRows(**{k: (None if getattr(good, k) is None else getattr(good, k).copy()) for k in rp.ARRAY_KEYS})
        for k, f in change.items():
            f(getattr(p, k))
        with pytest.raises(ValueError):
            host_unpack(p)

    def set_at(i, v):
        def f(a):
            a[i] = v
        return f

    broken(pi_idx=set_at(0, 4672))                                   # a column past the row
    broken(pi_idx=set_at(1, 0))                                      # columns that do not ascend
    broken(pi_off=set_at(3, 10 ** 6))                                # offsets past the entries
    broken(pi_off=set_at(0, 1))
    broken(mask_idx=set_at(0, 5000))
    broken(pos=lambda a: a.__setitem__((0, 101), 7))                 # a row kind out of range
    broken(pos=lambda a: a.__setitem__((0, 102), 0))                 # a row without a mask among rows with one
    broken(pos=lambda a: a.__setitem__((0, slice(0, 96)), 0))        # no men: no position
    broken(pos=lambda a: a.__setitem__((0, 99), 120))                # a half-move count above the cap
    assert all(rc.same_bits(g, w) for g, w in zip(host_unpack(good), (s, pi, z, mask)))


def test_sanitizer_build_over_seeded_rows():
    """The core as a stand-alone host program (its own main, never loaded into Python) under AddressSanitizer and
    UndefinedBehaviorSanitizer: 20 000 seeded rows, RAW rows and rows of 4672 entries among them, through the straight loops
    and the lane split, with exactly-sized buffers."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "rowpack_shim"), "../_build/rowpack_shim_san"])
    out = subprocess.run([os.path.join(HERE, "_build", "rowpack_shim_san")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    words = out.stdout.split()
    got = dict(zip(words[::2], (int(w) for w in words[1::2])))
    assert got["rows"] == 20000 and got["raw"] > 0 and got["full_pi"] > 0 and got["mask_list"] > 0 and got["mask_none"] > 0, got


# ---- files ------------------------------------------------------------------------------------------------------------------------
def _store(base):
    """A small store: two replay shards with masks (one with extra keys and z [n,1]), one without, one per-game file"""
    from matrix0_amd.data_writer import ShardIndex, write_npz
    s, pi, z, mask = rc.worker_rows()
    es, epi, ez, em, _ = rc.edge_rows(24, seed=2)
    ok = np.isfinite(epi).all(axis=1)
    shards = {"replays/replays_a.npz": dict(s=s[:50], pi=pi[:50], z=z[:50].reshape(-1, 1), legal_mask=mask[:50],
                                            meta_moves=np.array([50]), ssl_threat=np.ones((50, 8, 8), np.float32)),
              "replays/replays_b.npz": dict(s=s[50:90], pi=pi[50:90], z=z[50:90]),
              "replays/replays_c.npz": dict(s=es[ok], pi=epi[ok], z=ez[ok], legal_mask=em[ok]),
              "selfplay/selfplay_d.npz": dict(s=s[90:100], pi=pi[90:100], z=z[90:100], legal_mask=mask[90:100].astype(bool))}
    base.mkdir(parents=True, exist_ok=True)
    index = ShardIndex(base)
    for name, data in shards.items():
        (base / name).parent.mkdir(parents=True, exist_ok=True)
        write_npz(base / name, data)
        index.add(base / name, len(data["s"]), "selfplay")
    return shards


def _table(base):
    with sqlite3.connect(base / "data_metadata.db") as conn:
        return conn.execute("SELECT path, size_bytes, sample_count, checksum, source, corrupted FROM shards").fetchall()


def test_pack_then_unpack_of_a_store_restores_every_shard_and_keeps_the_table(tmp_path):
    shards = _store(tmp_path / "dense")
    assert rp.main(["pack", str(tmp_path / "dense"), str(tmp_path / "packed"), "--device", "host"]) == 0
    assert rp.main(["unpack", str(tmp_path / "packed"), str(tmp_path / "back"), "--device", "host"]) == 0
    for name, data in shards.items():
        with np.load(tmp_path / "packed" / name) as d:
            assert "rowpack_version" in d.files and not set(d.files) & {"s", "pi", "legal_mask"}
            for k in set(data) - set(rp.DENSE_KEYS):
                assert rc.same_bits(d[k], data[k]), (name, k)
        with np.load(tmp_path / "back" / name) as d:
            assert set(d.files) == set(data), name
            for k in data:
                assert rc.same_bits(d[k], data[k]), (name, k)
    for base in ("packed", "back"):
        rows = _table(tmp_path / base)
        assert len(rows) == 4
        for (path, size, count, checksum, source, corrupted), (name, data) in zip(rows, shards.items()):
            assert path == str(tmp_path / base / name) and count == len(data["s"]) and source == "selfplay" and not corrupted
            assert size == os.path.getsize(path) and checksum == hashlib.sha256(open(path, "rb").read()).hexdigest()
    info = rp.info(tmp_path / "packed")
    assert info["rows"] == sum(len(d["s"]) for d in shards.values()) and info["dense_shards"] == 0
    assert info["rows_by_kind"]["raw"] > 0 and info["masks_by_kind"]["list"] > 0 and info["packed_bytes_per_row"] < rp.DENSE_ROW_BYTES
    assert rp.info(tmp_path / "dense")["rows_by_kind"] == info["rows_by_kind"]


def test_the_reader_yields_the_same_samples_from_dense_packed_and_mixed_stores(tmp_path):
    from matrix0_amd.npz_dataset import ReplayReader
    shards = _store(tmp_path / "dense")
    rp._convert(tmp_path / "dense", tmp_path / "packed", True, "host")
    rp._convert(tmp_path / "dense", tmp_path / "mixed", True, "host")
    for name in list(shards)[::2]:                      # every other shard of the mixed store back to dense, in place
        rp.write_npz(tmp_path / "mixed" / name, rp.load_shard(tmp_path / "mixed" / name, device="host"))

    def stream(base):
        out = []
        for s, pi, z, lm in ReplayReader(str(tmp_path / base), seed=11).iter_samples(epochs=2):
            out.append(hashlib.sha256(s.tobytes() + pi.tobytes() + np.float32(z).tobytes() + (b"" if lm is None else lm.tobytes())).hexdigest())
        return out

    dense = stream("dense")
    assert len(dense) == 2 * sum(len(d["s"]) for d in shards.values())
    assert stream("packed") == dense and stream("mixed") == dense
    assert not any(r[5] for r in _table(tmp_path / "packed"))


def test_the_command_line_packs_one_shard_and_reports_it(tmp_path, capsys):
    import json
    shards = _store(tmp_path / "dense")
    src = tmp_path / "dense" / "replays" / "replays_a.npz"
    assert rp.main(["pack", str(src), str(tmp_path / "a_packed.npz"), "--device", "host"]) == 0
    capsys.readouterr()
    assert rp.main(["info", str(tmp_path / "a_packed.npz")]) == 0
    got = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert got["rows"] == 50 and got["rows_by_kind"] == {"packed": 50, "raw": 0} and got["masks_by_kind"]["legal"] == 50
    assert got["packed_bytes_per_row"] < 400 and got["dense_bytes_per_row"] == 28228
    back = rp.load_shard(tmp_path / "a_packed.npz", device="host")
    assert set(back) == set(shards["replays/replays_a.npz"]) and back["z"].shape == (50, 1)


def test_the_shard_writers_write_packed_shards_on_request(tmp_path):
    from matrix0_amd.data_writer import ReplayShardWriter, SelfplayShardWriter
    from matrix0_amd.npz_dataset import ReplayReader
    s, pi, z, mask = rc.worker_rows()
    games = [dict(s=s[a:b], pi=pi[a:b], z=z[a:b], legal_mask=mask[a:b], meta_moves=np.array([b - a]))
             for a, b in ((0, 16), (16, 40), (40, 75))]
    for packed in (False, True):
        w = ReplayShardWriter(str(tmp_path / f"replay_{packed}"), shard_size=32, packed=packed)
        for g in games:
            w.add_game(g)
        w.close()
        SelfplayShardWriter(str(tmp_path / f"replay_{packed}"), packed=packed).add_selfplay_data(games[0], 0, 0)
    dense, packed = ([r[0] for r in _table(tmp_path / f"replay_{p}")] for p in (False, True))          # in the order written
    assert len(dense) == len(packed) == 4
    loaded = lambda files: [rp.load_shard(f, device="host") for f in files]
    for d, p in zip(loaded(dense), loaded(packed)):
        assert set(d) == set(p)
        for k in d:
            assert rc.same_bits(d[k], p[k]), k
    assert all("rowpack_version" in np.load(f).files for f in packed) and not any("rowpack_version" in np.load(f).files for f in dense)
    counts = lambda base: sorted(r[2] for r in _table(tmp_path / base))
    assert counts("replay_True") == counts("replay_False") == [11, 16, 32, 32]
    assert len(list(ReplayReader(str(tmp_path / "replay_True"), seed=1).iter_samples(epochs=1))) == 91
    for r in _table(tmp_path / "replay_True"):
        assert r[1] == os.path.getsize(r[0]) and r[3] == hashlib.sha256(open(r[0], "rb").read()).hexdigest()


def test_the_selfplay_worker_builds_the_writer_its_key_names(tmp_path):
    from matrix0_amd import selfplay
    from matrix0_amd.data_writer import ReplayShardWriter, SelfplayShardWriter
    cfg = {"data_dir": str(tmp_path)}
    w = selfplay.shard_writer(cfg, {})
    assert type(w) is SelfplayShardWriter and not w.packed
    for key, packed in ((True, False), ("packed", True)):
        w = selfplay.shard_writer(cfg, {"replay_shards": key, "shard_size": 64, "max_shards": 3})
        assert type(w) is ReplayShardWriter and w.packed is packed and (w.shard_size, w.max_shards) == (64, 3)
    assert type(selfplay.shard_writer(cfg, {"replay_shards": False})) is SelfplayShardWriter


def test_reanalyse_of_a_packed_copy_equals_reanalyse_of_the_dense_shards(monkeypatch, tmp_path):
    """reanalyse_shards with the stand-in engine of tests/test_reanalyse.py behind the real Analyzer, over dense shards and over
    their packed copy: the same report and the same shards out"""
    import json
    from matrix0_amd import analysis, engine as eng, reanalyse
    from tests import test_reanalyse as tr
    fens, s, pi, z, mask = tr._rows()
    n = len(fens)
    (tmp_path / "dense").mkdir()
    for k, (a, b) in enumerate(((0, 7), (7, n))):
        np.savez_compressed(tmp_path / "dense" / f"shard_{k:03d}.npz", s=s[a:b], pi=pi[a:b], z=z[a:b].reshape(-1, 1), legal_mask=mask[a:b],
                            meta_row=np.arange(a, b, dtype=np.int32))
    assert rp.main(["pack", str(tmp_path / "dense"), str(tmp_path / "packed"), "--device", "host"]) == 0
    kinds = rp.info(tmp_path / "packed")
    assert kinds["rows"] == n and kinds["rows_by_kind"]["raw"] >= 1 and kinds["masks_by_kind"]["list"] >= 1
    monkeypatch.setattr(eng, "AnalysisEngine", tr._FakeEngine)
    out = {}
    for base in ("dense", "packed"):
        tr._FakeEngine.made = []
        rep = reanalyse.reanalyse_shards(tmp_path / base, tmp_path / ("out_" + base), analyzer=analysis.Analyzer(None, tr.CFG, slots=3),
                                         sims=16, first_id=1000)
        shards = [dict(np.load(sh["written"])) for sh in rep["shards"]]
        out[base] = (json.dumps({k: v for k, v in rep.items() if k != "shards"}, sort_keys=True),
                     [{k: v for k, v in sh.items() if k not in ("source", "written")} for sh in rep["shards"]], shards)
    assert out["dense"][0] == out["packed"][0] and out["dense"][1] == out["packed"][1]
    assert out["dense"][1][0]["rows"] == 7 and len(out["dense"][2]) == 2
    for d, p in zip(out["dense"][2], out["packed"][2]):
        assert set(d) == set(p) == {"s", "pi", "z", "legal_mask", "meta_row"}
        for k in d:
            assert rc.same_bits(d[k], p[k]), k
    assert not rc.same_bits(out["dense"][2][0]["pi"], pi[:7])                  # the rows were searched


def test_one_hot_rows_pack_without_their_pi_as_the_dense_rows_do():
    s, _, z, mask, kinds = rc.edge_rows(2 * rc.EDGES, seed=4)
    idx = (np.arange(len(s)) * 977 + 4671) % 4672
    idx[:3] = (0, 4671, 64)
    pi = np.zeros((len(s), 4672), np.float32)
    pi[np.arange(len(s)), idx] = 1.0
    for m in (mask, None):
        got, want = rp.pack_rows_onehot(s, idx, z, m, device="host"), host_pack(s, pi, z, m)
        assert rc.same_packed(got, want) is None, rc.same_packed(got, want)
        assert got.kinds()["rows"]["raw"] >= 2 and differs_from_ref(got, ref.pack_rows(s, pi, m)) is None
        assert all(rc.same_bits(g, w) for g, w in zip(host_unpack(got), (s, pi, z, m)))
    with pytest.raises(ValueError):
        rp.pack_rows_onehot(s, np.full(len(s), 4672), z, mask, device="host")


def test_arrays_of_the_wrong_type_or_length_never_reach_the_library(tmp_path):
    s, pi, z, mask = (a[:20] for a in rc.worker_rows())
    good = host_pack(s, pi, z, mask)
    changes = {"z": good.z[:-1], "pi_off": good.pi_off[:-1], "mask_off": good.mask_off.astype(np.int32), "pi_idx": good.pi_idx.astype(np.int32),
               "pi_val": good.pi_val[:-1], "pos": good.pos[:, :100], "raw_pi": np.zeros((1, 4672), np.float32),
               "raw_planes": np.zeros((0, 19, 64), np.float32), "pi_val ": good.pi_val.astype(np.float64),
               "z ": np.broadcast_to(good.z[:1], good.z.shape)}                     # not contiguous memory of its own
    for key, value in changes.items():
        p = rp.PackedRows(**{k: getattr(good, k) for k in rp.ARRAY_KEYS})
        setattr(p, key.strip(), value)
        with pytest.raises(ValueError, match="packed rows"):
            host_unpack(p)
    # the same through a file: a truncated key is a ValueError of load_shard, and the reader marks the shard, not the process
    d = rp.packed_to_dict(good)
    d["rowpack_pi_off"] = d["rowpack_pi_off"][:5]
    rp.write_npz(tmp_path / "bad.npz", d)
    with pytest.raises(ValueError, match="packed rows"):
        rp.load_shard(tmp_path / "bad.npz", device="host")


def test_files_are_told_apart_by_their_names_and_only_the_keys_asked_for_are_read(tmp_path, monkeypatch):
    from matrix0_amd.data_writer import ShardIndex
    from matrix0_amd.npz_dataset import ReplayReader
    s, pi, z, mask = (a[:12] for a in rc.worker_rows())
    base = tmp_path / "store"
    (base / "replays").mkdir(parents=True)
    # a dense shard with a key that cannot be read without pickle: the reader never touched such keys, and still does not
    np.savez_compressed(base / "replays" / "a.npz", s=s, pi=pi, z=z, legal_mask=mask, trace=np.array([{"a": 1}], dtype=object))
    np.savez_compressed(base / "notes.npz", note=np.arange(3))                   # no rows in it
    index = ShardIndex(base)
    index.add(base / "replays" / "a.npz", 12, "selfplay")
    reader = ReplayReader(str(base), seed=0)
    assert len(list(reader.iter_samples(epochs=1))) == 12 and not any(r[5] for r in _table(base))
    assert rp.read_shard(base / "replays" / "a.npz", keys=()) == (None, {})
    assert set(rp.load_shard(base / "replays" / "a.npz", keys=("s", "z", "absent"))) == {"s", "z"}
    # pack copies the file without rows through and reports it
    got = rp._convert(base / "replays" / "a.npz", tmp_path / "a_dense_copy.npz", False, "host")
    assert got == {"shards": 1, "without_rows": 0} and open(tmp_path / "a_dense_copy.npz", "rb").read() == open(base / "replays" / "a.npz", "rb").read()
    np.savez_compressed(base / "replays" / "a.npz", s=s, pi=pi, z=z, legal_mask=mask, meta_x=np.arange(2))
    index.add(base / "replays" / "a.npz", 12, "selfplay")
    assert rp._convert(base, tmp_path / "packed", True, "host") == {"shards": 2, "without_rows": 1}
    assert open(tmp_path / "packed" / "notes.npz", "rb").read() == open(base / "notes.npz", "rb").read()
    packed_keys = rp.load_shard(tmp_path / "packed" / "replays" / "a.npz", device="host", keys=("pi", "meta_x"))
    assert set(packed_keys) == {"pi", "meta_x"} and rc.same_bits(packed_keys["pi"], pi)
    assert rp._convert(tmp_path / "packed", tmp_path / "packed2", True, "host") == {"shards": 2, "without_rows": 1}       # already packed: copied
    assert [r[2] for r in _table(tmp_path / "packed2")] == [12]
