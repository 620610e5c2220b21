"""The trainer's flip and rotate augmentations without a GPU: the core's tables against the reference's permutations
(tests/golden/ref_augment_perm.json), the host build of matrix0_amd/csrc/augment_core.h against the numpy restatement of the trainer
(tests/augment_ref.py), what the file mirror means in the project's own move encoding (the host rules build of tests/host_shim.py),
and matrix0_amd/score.py's aggregation of the three kinds on a stand-in backend."""
import ctypes as C
import json

import numpy as np
import pytest

from matrix0_amd import _abi
from matrix0_amd import score as sc
from matrix0_amd.data_writer import ShardIndex, write_npz
from tests import augment_ref as ref
from tests import augment_shim as shim
from tests import host_shim
from tests import rules_cases

N = 4672
RAYS, KNIGHTS, UNDER = range(0, 56), range(56, 64), range(64, 73)


# ---- (1) the tables ---------------------------------------------------------------------------------------------------------------
def test_the_constants_are_the_headers():
    assert _abi.AUGMENT_KINDS == ref.KINDS == {"none": 0, "hflip": 1, "rot180": 2}


@pytest.mark.parametrize("kind", ["hflip", "rot180"])
def test_core_tables_equal_the_reference_entry_for_entry(kind):
    perm, squares = shim.tables(ref.KINDS[kind])
    want = ref.perms()[ref.KINDS[kind]]
    assert perm.tolist() == want.tolist()
    assert sorted(perm.tolist()) == list(range(73)) and perm[perm].tolist() == list(range(73)), "an involution"
    for block in (RAYS, KNIGHTS, UNDER):
        assert sorted(perm[list(block)].tolist()) == list(block), "rays to rays, knights to knights, under-promotions to under-promotions"
    assert (perm[:56] % 7 == np.arange(56) % 7).all(), "a ray keeps its step"
    assert perm[[64, 67, 70]].tolist() == [64, 67, 70], "forward stays forward"
    sq = np.arange(64)
    want_sq = (sq // 8) * 8 + 7 - sq % 8 if kind == "hflip" else (7 - sq // 8) * 8 + 7 - sq % 8
    assert squares.tolist() == want_sq.tolist() and squares[squares].tolist() == sq.tolist()
    k = ref.KINDS[kind]
    cols = np.array([shim.load().as_source_column(k, c) for c in range(N)])
    assert (cols == np.repeat(squares, 73) * 73 + np.tile(perm, 64)).all()


def test_the_identity_kind_and_what_is_no_kind():
    perm, squares = shim.tables(0)
    assert perm.tolist() == list(range(73)) and squares.tolist() == list(range(64))
    for bad in (-1, 3, 255):
        with pytest.raises(ValueError):
            shim.tables(bad)


# ---- (2) the host build against the numpy restatement ----------------------------------------------------------------------------
def rows(B, P=19, seed=0):
    """random bit patterns for s and pi (NaNs of every payload, infinities, denormals, both zeros among them) and a 0/1 mask"""
    rng = np.random.default_rng(seed + B)
    s = rng.integers(0, 2 ** 32, size=(B, P, 8, 8), dtype=np.uint32).view(np.float32)
    pi = rng.integers(0, 2 ** 32, size=(B, N), dtype=np.uint32).view(np.float32)
    mask = (rng.random((B, N)) < 0.1).astype(np.uint8)
    return s, pi, mask


def mixed_kinds(B, last):
    """kinds in a seeded mix, the last row taking `last`"""
    kinds = np.random.default_rng(B).integers(0, 3, size=B).astype(np.uint8)
    kinds[-1] = last
    return kinds


def same_bits(got, want):
    return all((a is None and b is None) or (a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes())
               for a, b in zip(got, want))


@pytest.mark.parametrize("B", [1, 3, 65])
def test_core_equals_the_reference_bit_for_bit(B):
    s, pi, mask = rows(B)
    for last in range(3):
        kinds = mixed_kinds(B, last)
        for m in (mask, None):
            got = shim.augment_rows(s, pi, m, kinds)
            assert same_bits(got, ref.augment(s, pi, m, kinds)), (B, last, m is None)
            assert same_bits(shim.augment_rows(*got, kinds), (s, pi, m)), "a kind applied twice returns the input"
    for name, k in ref.KINDS.items():
        assert same_bits(shim.augment_rows(s, pi, mask, np.full(B, k, np.uint8)), ref.augment(s, pi, mask, name)), name
    assert same_bits(shim.augment_rows(s, pi, mask, np.zeros(B, np.uint8)), (s, pi, mask))
    assert not same_bits(shim.augment_rows(s, pi, mask, np.ones(B, np.uint8)), (s, pi, mask))


def test_core_takes_other_plane_counts_and_refuses_what_the_abi_refuses():
    s, pi, mask = rows(3, P=5)
    kinds = np.array([2, 1, 0], np.uint8)
    assert same_bits(shim.augment_rows(s, pi, mask, kinds), ref.augment(s, pi, mask, kinds))
    with pytest.raises(ValueError):
        shim.augment_rows(s, pi, mask, np.array([0, 3, 1], np.uint8))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    f = shim.load().as_augment_rows
    so, po, mo = np.empty_like(s), np.empty_like(pi), np.empty_like(mask)
    assert f(p(s), 5, p(pi), p(mask), p(kinds), 3, p(so), p(po), p(mo)) == 0
    assert f(p(s), 5, p(pi), p(mask), p(kinds), 3, p(so), p(po), None) == -1
    assert f(p(s), 5, p(pi), None, p(kinds), 3, p(so), p(po), p(mo)) == -1
    assert f(p(s), 5, p(pi), None, p(kinds), 0, p(so), p(po), None) == -1
    assert f(p(s), 0, p(pi), None, p(kinds), 3, p(so), p(po), None) == -1
    assert f(p(s), 5, p(pi), None, p(kinds), 3, p(s), p(po), None) == -1, "in place"


# ---- (3) what the file mirror means in the project's own move encoding -------------------------------------------------------------
# every root of tests/rules_cases.py with its castling rights stripped, two under-promotion positions with captures to both sides, and
# two with the seven-step moves towards the west and along the long diagonals that the roots lack
UNDER_PROMOTIONS = ["1n1n3k/2P5/8/8/8/8/8/K7 w - - 0 1", "k7/8/8/8/8/8/2p5/1N1N3K b - - 0 1"]
LONG_RAYS = ["1K6/8/8/3k4/8/8/7R/Q7 w - - 0 1", "7Q/8/8/8/1k6/8/3K4/7Q w - - 0 1"]


def without_castling(fen):
    f = fen.split(" ")
    f[2] = "-"
    return " ".join(f)


def file_mirror(fen):
    """the position with its files mirrored (a <-> h); it has no castling rights"""
    board, turn, castling, ep, half, full = fen.split(" ")
    assert castling == "-"
    ep = "-" if ep == "-" else "abcdefgh"[7 - "abcdefgh".index(ep[0])] + ep[1]
    return " ".join(["/".join(r[::-1] for r in board.split("/")), turn, "-", ep, half, full])


def legal(fen):
    """{move as from | to << 8 | promotion << 16: policy index} by the host build of the device's rules"""
    mv, idx = np.zeros(256, np.int32), np.zeros(256, np.int32)
    n = host_shim.load("chess").hc_legal(fen.encode(), mv.ctypes.data_as(C.c_void_p), idx.ctypes.data_as(C.c_void_p))
    assert n >= 0, fen
    return dict(zip(mv[:n].tolist(), idx[:n].tolist()))


def test_hflip_is_the_file_mirror_in_the_projects_move_encoding_on_all_73_channels():
    fens = [without_castling(f) for _, _, f in rules_cases.ROOTS] + UNDER_PROMOTIONS + LONG_RAYS
    seen, disagree = set(), set()
    for fen in fens:
        moves, mirrored = legal(fen), legal(file_mirror(fen))
        if not moves:
            assert not mirrored
            continue
        index = np.array(list(moves.values()))
        mask = np.zeros((1, N), np.uint8)
        mask[0, index] = 1
        onehot = np.zeros((len(moves), N), np.float32)
        onehot[np.arange(len(moves)), index] = 1.0
        s = np.zeros((len(moves), 1, 8, 8), np.float32)
        _, got_pi, got_mask = shim.augment_rows(s, onehot, np.repeat(mask, len(moves), axis=0), np.ones(len(moves), np.uint8))
        want_mask = np.zeros(N, np.uint8)
        want_mask[list(mirrored.values())] = 1
        assert (got_mask[0] == want_mask).all(), fen
        for row, (m, i) in enumerate(moves.items()):
            mm = ((m & 255) ^ 7) | (((m >> 8) & 255) ^ 7) << 8 | (m >> 16) << 16
            assert mm in mirrored, (fen, m)
            seen.add(i % 73)
            if np.flatnonzero(got_pi[row]).tolist() != [mirrored[mm]]:
                disagree.add(i % 73)
    assert seen == set(range(73)), sorted(set(range(73)) - seen)
    assert disagree == set(), "the reference's horizontal-flip table and the move encoding disagree on these channels"


# ---- (4) score.py's aggregation ------------------------------------------------------------------------------------------------------
class KindBackend:
    """A stand-in for M0Backend: a row's policy loss is 1 + its first plane cell, scaled by 1 (none), 2 (hflip) or 4 (rot180); its
    value loss 0.5 times that.  Counts its calls per kind."""

    def __init__(self):
        self.calls = []

    def score(self, s, pi, z, legal_mask=None, *, mask_mode=None, label_smoothing=0.0, value_loss="mse", huber_delta=1.0,
              augment=None):
        self.calls.append(augment if augment is None or isinstance(augment, str) else "per-row")
        n = len(s)
        kinds = np.zeros(n, np.int64) if augment is None else \
            np.full(n, _abi.AUGMENT_KINDS[augment]) if isinstance(augment, str) else np.asarray(augment, np.int64)
        rows = np.zeros((n, 8), np.float32)
        rows[:, 0] = (1.0 + np.asarray(s)[:, 0, 0, 0]) * np.array([1.0, 2.0, 4.0])[kinds]
        rows[:, 2] = 0.5 * rows[:, 0]
        rows[:, 4] = 1.0
        return rows

    def close(self):
        pass


@pytest.fixture()
def store(tmp_path):
    rng = np.random.default_rng(5)
    base = []
    index = ShardIndex(tmp_path)
    for name, n in (("a.npz", 5), ("b.npz", 6)):
        s = np.zeros((n, 19, 8, 8), np.float32)
        s[:, 0, 0, 0] = rng.random(n).astype(np.float32)
        pi = np.zeros((n, N), np.float32)
        pi[np.arange(n), rng.integers(0, N, n)] = 0.5
        pi[np.arange(n), rng.integers(0, N, n)] += 0.5
        write_npz(tmp_path / name, {"s": s, "pi": pi, "z": np.ones(n, np.float32)})
        index.add(tmp_path / name, n, "selfplay")
        base.append(1.0 + s[:, 0, 0, 0].astype(np.float64))
    return tmp_path, np.concatenate(base)


def test_trainer_weights_follow_the_trainers_elif_chain():
    assert sc.trainer_weights() == sc.trainer_weights(True) == {"hflip": 0.5, "rot180": 0.25, "none": 0.25}
    assert sc.trainer_weights(False) == {"hflip": 0.5, "rot180": 0.0, "none": 0.5}


@pytest.mark.parametrize("rot180", [True, False])
def test_trainer_report_weighs_the_three_kinds(store, rot180, tmp_path):
    path, base = store
    be = KindBackend()
    per = tmp_path / "per.npz"
    r = sc.score_shards(path, be, batch=4, augment="trainer", augment_rotate180=rot180, per_sample=str(per))
    assert be.calls == ["none", "none", "hflip", "hflip", "rot180", "rot180"] * 2
    x = r["augment"]
    assert x["mode"] == "trainer" and x["weights"] == ({"none": 0.25, "hflip": 0.5, "rot180": 0.25} if rot180 else
                                                       {"none": 0.5, "hflip": 0.5, "rot180": 0.0})
    mean = base.mean()
    for k, scale in (("none", 1.0), ("hflip", 2.0), ("rot180", 4.0)):
        assert x["by_kind"][k]["rows"] == 11
        assert x["by_kind"][k]["policy_loss"] == pytest.approx(scale * mean, rel=1e-6)
        assert x["by_kind"][k]["value_loss"] == pytest.approx(0.5 * scale * mean, rel=1e-6)
    want = (0.5 * 2.0 + 0.25 * 4.0 + 0.25 * 1.0 if rot180 else 0.5 * 2.0 + 0.5 * 1.0) * mean
    assert x["expected"]["policy_loss"] == pytest.approx(want, rel=1e-6)
    assert x["expected"]["value_loss"] == pytest.approx(0.5 * want, rel=1e-6)
    assert x["expected"]["total"] == pytest.approx(1.5 * want, rel=1e-6)
    # the weighted sum of the report's own per-kind means, exactly
    for key in ("policy_loss", "value_loss", "total"):
        assert x["expected"][key] == pytest.approx(sum(x["weights"][k] * x["by_kind"][k][key] for k in x["weights"]), rel=1e-12)
    gap = x["symmetry_gap"]
    assert gap["rows"] == 11 and gap["policy_loss"]["mean"] == pytest.approx(mean, rel=1e-6)
    assert gap["policy_loss"]["max"] == pytest.approx(base.max(), rel=1e-6) and gap["value_loss"]["max"] == pytest.approx(0.5 * base.max(), rel=1e-6)
    # the figures at the top are those of "none"; every shard carries its own block
    assert r["policy_loss"] == x["by_kind"]["none"]["policy_loss"]
    assert [v["augment"]["by_kind"]["hflip"]["rows"] for v in r["by_shard"].values()] == [5, 6]
    with np.load(per) as f:
        assert set(f.files) >= {"columns", "columns_none", "columns_hflip", "columns_rot180"}
        assert np.array_equal(f["columns"], f["columns_none"]) and np.array_equal(f["columns_hflip"][:, 0], 2 * f["columns_none"][:, 0])


def test_one_kind_and_no_kind(store, tmp_path):
    path, base = store
    be = KindBackend()
    plain = sc.score_shards(path, be, batch=16)
    assert be.calls == [None, None] and "augment" not in plain and all("augment" not in v for v in plain["by_shard"].values())
    be = KindBackend()
    r = sc.score_shards(path, be, batch=16, augment="hflip")
    assert be.calls == ["hflip", "hflip"] and r["augment"] == {"mode": "hflip"}
    assert r["policy_loss"] == pytest.approx(2 * plain["policy_loss"], rel=1e-6)
    # score_arrays: a per-row array is cut with the chunks; "trainer" stacks the three kinds
    s = np.zeros((5, 19, 8, 8), np.float32)
    pi = np.zeros((5, N), np.float32)
    pi[:, 7] = 1.0
    kinds = np.array([0, 1, 2, 1, 0], np.uint8)
    be = KindBackend()
    got = sc.score_arrays(be, s, pi, np.zeros(5, np.float32), batch=2, augment=kinds)
    assert got[:, 0].tolist() == [1.0, 2.0, 4.0, 2.0, 1.0] and be.calls == ["per-row"] * 3
    three = sc.score_arrays(be, s, pi, np.zeros(5, np.float32), batch=2, augment="trainer")
    assert three.shape == (3, 5, 8) and three[:, 0, 0].tolist() == [1.0, 2.0, 4.0]
    for bad in ("vflip", np.zeros(4, np.uint8)):
        with pytest.raises(ValueError):
            sc.score_arrays(be, s, pi, np.zeros(5, np.float32), augment=bad)


def test_ssl_with_an_augmentation_is_refused(store, tmp_path, capsys):
    path, _ = store
    s, pi, z = np.zeros((2, 19, 8, 8), np.float32), np.zeros((2, N), np.float32), np.zeros(2, np.float32)
    for kind in ("hflip", "rot180", "trainer", np.ones(2, np.uint8)):
        with pytest.raises(ValueError, match="ssl"):
            sc.score_arrays(KindBackend(), s, pi, z, ssl="planes", augment=kind)
    for kind in ("hflip", "trainer"):
        with pytest.raises(ValueError, match="ssl"):
            sc.score_shards(path, KindBackend(), ssl="planes", augment=kind)
    cfg = tmp_path / "config.json"
    cfg.write_text(json.dumps({"model": {"planes": 19}}))
    with pytest.raises(SystemExit) as e:
        sc.main(["--config", str(cfg), "--checkpoint", "A.pt", "--data", str(path), "--ssl", "--augment", "hflip"])
    assert e.value.code == 2 and "--ssl cannot be combined with --augment" in capsys.readouterr().err


def test_command_line_prints_the_trainer_line_and_reads_the_rotate_switch(store, tmp_path, monkeypatch, capsys):
    path, base = store
    monkeypatch.setattr(sc, "load_backend", lambda model_cfg, ckpt, device: KindBackend())
    out = tmp_path / "report.json"
    for rot180, want in ((True, 2.25), (False, 1.5)):
        cfg = tmp_path / f"config_{rot180}.json"
        cfg.write_text(json.dumps({"model": {"planes": 19}, "training": {"augment_rotate180": rot180}}))
        assert sc.main(["--config", str(cfg), "--checkpoint", "A.pt", "--data", str(path), "--augment", "trainer", "--json", str(out)]) == 0
        lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
        assert len(lines) == 2 and "augment trainer" in lines[1] and "symmetry gap" in lines[1] and "expected" in lines[1]
        rep = json.loads(out.read_text())
        assert rep["augment_options"] == {"augment": "trainer", "augment_rotate180": rot180}
        assert rep["checkpoints"]["A.pt"]["augment"]["expected"]["policy_loss"] == pytest.approx(want * base.mean(), rel=1e-6)
    cfg = tmp_path / "config.json"
    cfg.write_text(json.dumps({"model": {"planes": 19}}))
    assert sc.main(["--config", str(cfg), "--checkpoint", "A.pt", "--data", str(path), "--json", str(out)]) == 0
    assert len([ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]) == 1
    rep = json.loads(out.read_text())
    assert "augment_options" not in rep and "augment" not in rep["checkpoints"]["A.pt"]
