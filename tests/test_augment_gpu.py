"""The trainer's augmentations on the device: augment_rows_kernel through m0_augment_rows (encoding.augment) against the numpy
restatement of the trainer (tests/augment_ref.py) bit for bit, m0_net_score_aug (M0Backend.score(augment=...)) against the plain
score of rows transformed on the host, its row independence, and score_shards(augment="trainer") with the real backend."""
import numpy as np
import pytest

from matrix0_amd import _abi
from matrix0_amd import encoding as enc
from oracle import net_layers as nl
from tests import augment_ref as ref
from tests import net_layer_cases as net_cases
from tests.test_augment import mixed_kinds, rows, same_bits
from tests.test_score_gpu import OPTS, SMALL, _targets

pytestmark = pytest.mark.gpu

N = 4672


def special_rows(B, P=19):
    """random bit patterns with, in every row, a negative zero, denormals of both signs, infinities and NaNs of several payloads"""
    s, pi, mask = rows(B, P, seed=11)
    bits = pi.view(np.uint32)
    bits[:, 0], bits[:, 72], bits[:, 73], bits[:, N - 1] = 0x80000000, 0x00000001, 0x807fffff, 0x7fc00001
    bits[:, 2000], bits[:, 2001], bits[:, 2002] = 0xffc12345, 0x7f800000, 0x7f800001
    s.view(np.uint32)[:, 0, 0, 0] = 0x7fa00000
    return s, pi, mask


# ---- (6) the kernel against the reference ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, 65, 257])
def test_kernel_equals_the_reference_bit_for_bit(B):
    s, pi, mask = special_rows(B)
    for last in range(3):
        kinds = mixed_kinds(B, last)
        for m in (mask, None):
            got = enc.augment(s, pi, m, kinds)
            want = ref.augment(s, pi, m, kinds)
            assert same_bits(got, want), (B, last, m is None)
    for name in ref.KINDS:
        assert same_bits(enc.augment(s, pi, mask, name), ref.augment(s, pi, mask, name)), name
    again = enc.augment(*enc.augment(s, pi, mask, "rot180"), "rot180")
    assert same_bits(again, (s, pi, mask))


def test_kernel_walks_more_rows_than_its_grid_and_takes_other_plane_counts():
    B = 2048 + 3                                        # the grid is capped at 2048 workgroups: the last rows are second visits
    s, pi, mask = rows(B, P=5, seed=3)
    kinds = mixed_kinds(B, 2)
    kinds[2048:] = [1, 0, 2]
    assert same_bits(enc.augment(s, pi, mask, kinds), ref.augment(s, pi, mask, kinds))


def test_python_wrapper_checks_its_arguments():
    s, pi, mask = rows(2)
    for bad in ("vflip", np.array([0, 3]), np.array([0, 1, 2]), np.array([0.0, 1.0])):
        with pytest.raises(ValueError):
            enc.augment(s, pi, mask, bad)
    with pytest.raises(ValueError):
        enc.augment(s, pi[:, :100], None, "hflip")
    with pytest.raises(ValueError):
        enc.augment(s, pi, mask[:1], "hflip")
    assert enc.AUGMENT_KINDS == _abi.AUGMENT_KINDS
    got = enc.augment(s, pi, mask.astype(bool), "hflip")
    assert got[2].dtype == np.uint8 and same_bits(got, ref.augment(s, pi, mask, "hflip"))


# ---- (7)-(9) behind a forward -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_net():
    from matrix0_amd.backend import M0Backend
    be = M0Backend.from_state_dict(SMALL, net_cases.weights(SMALL, sharp=True))
    yield be
    be.close()


@pytest.fixture(scope="module")
def stored():
    """B -> (s, pi, z, mask): planes as the network's tests draw them, targets as tests/test_score_gpu.py makes them"""
    out = {}
    for B in (5, 65):
        pi, z, mask = _targets(9, B)
        out[B] = (nl.random_planes(B, 5).numpy().astype(np.float32), pi, z, mask)
    return out


@pytest.mark.parametrize("B", [5, 65])
@pytest.mark.parametrize("mode", ["legal", "target", "none"])
def test_score_under_a_kind_is_the_score_of_the_transformed_rows(small_net, stored, mode, B):
    be = small_net
    s, pi, z, mask = stored[B]
    if mode != "legal":
        mask = None
    for name, o in OPTS.items():
        for kind in ("hflip", "rot180", mixed_kinds(B, 1)):
            got = be.score(s, pi, z, mask, mask_mode=mode, augment=kind, **o)
            s2, pi2, m2 = ref.augment(s, pi, mask, kind)
            want = be.score(s2, pi2, z, m2, mask_mode=mode, **o)
            assert got.shape == (B, 8) and got.tobytes() == want.tobytes(), (name, kind if isinstance(kind, str) else "mixed")
    assert {(o["label_smoothing"], o["value_loss"]) for o in OPTS.values()} >= {(0.0, "mse"), (0.05, "huber")}


def test_no_augmentation_and_the_identity_are_todays_score(small_net, stored):
    import ctypes as C
    from matrix0_amd import _lib
    from matrix0_amd.backend import score_opts
    be = small_net
    for B in (5, 65):
        s, pi, z, mask = stored[B]
        for o in OPTS.values():
            today = np.empty((B, 8), np.float32)
            opts = score_opts("legal", o["label_smoothing"], o["value_loss"], o["huber_delta"])
            assert _lib.lib().m0_net_score(be.handle, _lib.ptr(s), _lib.ptr(pi), _lib.ptr(z), _lib.ptr(mask), B, C.byref(opts),
                                           _lib.ptr(today)) == _abi.M0_OK
            assert be.score(s, pi, z, mask, **o).tobytes() == today.tobytes()
            assert be.score(s, pi, z, mask, augment=None, **o).tobytes() == today.tobytes()
            assert be.score(s, pi, z, mask, augment="none", **o).tobytes() == today.tobytes()
            assert be.score(s, pi, z, mask, augment=np.zeros(B, np.uint8), **o).tobytes() == today.tobytes()
    with pytest.raises(ValueError):
        be.score(s, pi, z, mask, augment="trainer")
    with pytest.raises(ValueError):
        be.score(s, pi, z, mask, augment=np.full(B, 3))


def test_a_rows_score_under_its_kind_does_not_depend_on_its_neighbours(small_net, stored):
    be = small_net
    B = 65
    s, pi, z, mask = stored[B]
    o = dict(label_smoothing=0.05, value_loss="huber", huber_delta=0.5)
    uniform = [be.score(s, pi, z, mask, augment=k, **o) for k in ("none", "hflip", "rot180")]
    assert not np.array_equal(uniform[0], uniform[1]) and not np.array_equal(uniform[0], uniform[2])
    for last in range(3):
        kinds = mixed_kinds(B, last)
        got = be.score(s, pi, z, mask, augment=kinds, **o)
        for b in range(B):
            assert got[b].tobytes() == uniform[kinds[b]][b].tobytes(), (last, b)


# ---- (10) the shard walk --------------------------------------------------------------------------------------------------------
def test_score_shards_trainer_is_the_weighted_sum_of_three_runs(small_net, tmp_path):
    from matrix0_amd import score as sc
    from matrix0_amd.data_writer import ShardIndex, write_npz
    from tests.test_score import _shard
    be = small_net
    rng = np.random.default_rng(4)
    x = nl.random_planes(13, 6).numpy().astype(np.float32)
    index = ShardIndex(tmp_path)
    for name, d, part in (("a_masked.npz", _shard(rng, 6, "masked"), x[:6]), ("b_soft.npz", _shard(rng, 7, "soft"), x[6:])):
        d["s"] = np.ascontiguousarray(part)
        write_npz(tmp_path / name, d)
        index.add(tmp_path / name, len(d["z"]), "selfplay")
    opts = dict(label_smoothing=0.05, value_loss="huber", huber_delta=0.5)
    single = {k: sc.score_shards(tmp_path, be, batch=4, augment=k, **opts) for k in ("none", "hflip", "rot180")}
    plain = sc.score_shards(tmp_path, be, batch=4, **opts)
    assert {k: v for k, v in single["none"].items() if k != "augment"} == plain and "augment" not in plain
    for rot180, w in ((True, {"hflip": 0.5, "rot180": 0.25, "none": 0.25}), (False, {"hflip": 0.5, "rot180": 0.0, "none": 0.5})):
        r = sc.score_shards(tmp_path, be, batch=4, augment="trainer", augment_rotate180=rot180, **opts)
        x = r["augment"]
        assert x["weights"] == w and r["rows"] == 13 and r["scored"] == 13
        for k in w:
            assert x["by_kind"][k] == {key: v for key, v in single[k].items() if key in x["by_kind"][k]}, k
        for key in ("policy_loss", "value_loss", "total"):
            assert x["expected"][key] == pytest.approx(sum(w[k] * single[k][key] for k in w), rel=1e-12, abs=0), key
        gap = x["symmetry_gap"]
        print("symmetry gap of a random network:", gap)
        assert gap["rows"] == 13
        assert gap["policy_loss"]["mean"] > 0 and gap["policy_loss"]["max"] > 0
        assert gap["value_loss"]["mean"] > 0 and gap["value_loss"]["max"] > 0
        assert gap["policy_loss"]["max"] >= gap["policy_loss"]["mean"]
