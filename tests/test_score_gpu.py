"""The training-loss score on the device: score_rows_kernel through m0_score_rows against the float64 reference on the case set
and for its determinism, the argument checks, m0_net_score behind a real forward (M0Backend.score), and score_shards with the
real backend.  Every test appends the largest error per column it saw to tests/_build/score_parity.jsonl."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from matrix0_amd import _abi, _lib
from tests import net_layer_cases as net_cases
from tests import score_cases as cases
from tests import score_ref as ref

pytestmark = pytest.mark.gpu

GROUPS = {g["name"]: g for g in cases.groups()}
OPTS = {f"smooth{o['label_smoothing']}_{o['value_loss']}": o for o in cases.OPTION_SETS}
BATCHES = (1, 3, 5, 65)          # ROWS_PER_WG is 4: one partial workgroup, whole ones and a partial last one
PARITY_LOG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_build", "score_parity.jsonl")
SENTINEL = -7.0


def _log(test, worst, **more):
    os.makedirs(os.path.dirname(PARITY_LOG), exist_ok=True)
    with open(PARITY_LOG, "a") as f:
        f.write(json.dumps(dict(test=test, error_over_tolerance=dict(zip(_abi.SCORE_COLUMNS, np.asarray(worst).tolist())), **more)) + "\n")


def _opts(mask_mode, label_smoothing=0.0, value_loss="mse", huber_delta=1.0):
    mode = _abi.SCORE_MASK[mask_mode] if isinstance(mask_mode, str) else mask_mode
    return _abi.ScoreOpts(mode, label_smoothing, int(value_loss == "huber"), huber_delta)


def score_rows_rc(logits, value, pi, z, mask, B, opts):
    """m0_score_rows on arrays that may be None: (return code, rows prefilled with SENTINEL)"""
    rows = np.full((max(B, 1), _abi.SCORE_COLS), SENTINEL, np.float32)
    rc = _lib.lib().m0_score_rows(0, _lib.ptr(logits), _lib.ptr(value), _lib.ptr(pi), _lib.ptr(z), _lib.ptr(mask), B,
                                  C.byref(opts) if opts is not None else None, _lib.ptr(rows))
    return rc, rows


def score_rows(arrays, mask_mode, **o):
    rc, rows = score_rows_rc(*arrays, len(arrays[0]), _opts(mask_mode, **o))
    assert rc == _abi.M0_OK, _lib.last_error()
    return rows


# ---- (1) the kernel against the reference, and its determinism ----------------------------------------------------------------
@pytest.mark.parametrize("opts", OPTS)
@pytest.mark.parametrize("group", GROUPS)
def test_kernel_matches_the_reference_and_a_row_depends_on_itself_alone(group, opts):
    g, o = GROUPS[group], OPTS[opts]
    n = len(g["names"])
    want = ref.score_rows(g["logits"], g["value"], g["pi"], g["z"], g["mask"], mask_mode=g["mask_mode"], **o)
    first = {}                                          # case row -> the bits of its first result
    worst = np.zeros(_abi.SCORE_COLS)
    for B in BATCHES:
        for shift in (0, 3):                            # the same rows at other row indices
            arrays, idx = cases.tiled(g, B, shift)
            got = score_rows(arrays, g["mask_mode"], **o)
            worst = np.maximum(worst, ref.compare(got, want[idx]))
            for b, k in enumerate(idx):
                bits = got[b].tobytes()
                assert first.setdefault(int(k), bits) == bits, (g["names"][k], B, shift, b)
    arrays, idx = cases.tiled(g, 65)
    assert np.array_equal(score_rows(arrays, g["mask_mode"], **o), score_rows(arrays, g["mask_mode"], **o))
    assert len(first) == n
    print(group, opts, "largest error / tolerance per column:", np.round(worst, 5).tolist())
    _log(f"kernel:{group}:{opts}", worst)
    assert (worst <= 1.0).all(), dict(zip(_abi.SCORE_COLUMNS, worst.tolist()))


# ---- (2) argument checks -------------------------------------------------------------------------------------------------------
def _refused(rc, rows):
    return rc == _abi.M0_ERR_INVALID and (rows == SENTINEL).all()


def test_invalid_arguments_are_refused_and_touch_nothing():
    (logits, value, pi, z, mask), _ = cases.tiled(GROUPS["legal"], 3)
    good = _opts("legal")
    assert score_rows_rc(logits, value, pi, z, mask, 3, good)[0] == _abi.M0_OK
    assert _lib.lib().m0_score_rows(0, _lib.ptr(logits), _lib.ptr(value), _lib.ptr(pi), _lib.ptr(z), _lib.ptr(mask), 3,
                                    C.byref(good), None) == _abi.M0_ERR_INVALID
    for k in range(4):                                  # a null pointer among logits, value, pi, z
        args = [logits, value, pi, z]
        args[k] = None
        assert _refused(*score_rows_rc(*args, mask, 3, good)), k
    assert _refused(*score_rows_rc(logits, value, pi, z, mask, 3, None))
    for B in (0, -1):
        assert _refused(*score_rows_rc(logits, value, pi, z, mask, B, good)), B
    assert _refused(*score_rows_rc(logits, value, pi, z, None, 3, good)), "legal without a mask"
    for bad in (_opts(3), _opts(-1), _opts("legal", label_smoothing=1.0), _opts("legal", label_smoothing=-0.01),
                _opts("legal", label_smoothing=float("nan")), _opts("legal", huber_delta=0.0), _opts("legal", huber_delta=-2.0),
                _opts("target", huber_delta=float("nan"))):
        assert _refused(*score_rows_rc(logits, value, pi, z, mask, 3, bad)), (bad.mask_mode, bad.label_smoothing, bad.huber_delta)
    # the other modes take a null mask
    assert score_rows_rc(logits, value, pi, z, None, 3, _opts("target"))[0] == _abi.M0_OK
    assert score_rows_rc(logits, value, pi, z, None, 3, _opts("none"))[0] == _abi.M0_OK


# ---- (3) behind a forward ------------------------------------------------------------------------------------------------------
SMALL = dict(planes=19, channels=64, blocks=2, attention_heads=4, policy_size=4672, norm="group", activation="silu", preact=True,
             policy_factor_rank=32, self_supervised=False)


def _targets(seed, B):
    rng = np.random.default_rng(seed)
    pi = np.zeros((B, cases.N), np.float32)
    mask = np.zeros((B, cases.N), np.uint8)
    for b in range(B):
        cols = rng.choice(cases.N, size=20 + 7 * b, replace=False)
        mask[b, cols] = 1
        w = rng.dirichlet(np.full(6, 0.5)).astype(np.float32)
        pi[b, cols[:6]] = w
    return pi, np.array([(-1.0, 0.0, 1.0)[b % 3] for b in range(B)], np.float32), mask


@pytest.fixture(scope="module")
def small_net():
    from matrix0_amd.backend import M0Backend
    sd = net_cases.weights(SMALL, sharp=True)
    be = M0Backend.from_state_dict(SMALL, sd)
    yield be, sd, net_cases.planes().numpy().astype(np.float32)
    be.close()


@pytest.mark.parametrize("opts", OPTS)
@pytest.mark.parametrize("mode", ["legal", "target", "none"])
def test_backend_score_is_the_kernel_on_the_forwards_own_logits(small_net, mode, opts):
    be, _, x = small_net
    o = OPTS[opts]
    pi, z, mask = _targets(9, len(x))
    if mode != "legal":
        mask = None
    logits, value = be.infer_np(x)
    got = be.score(x, pi, z, mask, mask_mode=mode, **o)
    assert got.shape == (len(x), 8) and got.dtype == np.float32
    assert np.array_equal(got, score_rows((logits, value, pi, z, mask), mode, **o)), "the device logits are not the forward's"
    worst = ref.compare(got, ref.score_rows(logits, value, pi, z, mask, mask_mode=mode, **o))
    _log(f"backend:{mode}:{opts}", worst)
    assert (worst <= 1.0).all(), dict(zip(_abi.SCORE_COLUMNS, worst.tolist()))


def test_backend_score_resolves_the_mode_and_checks_its_arguments(small_net):
    be, _, x = small_net
    pi, z, mask = _targets(9, len(x))
    assert np.array_equal(be.score(x, pi, z, mask), be.score(x, pi, z, mask, mask_mode="legal"))
    assert np.array_equal(be.score(x, pi, z), be.score(x, pi, z, mask_mode="target"))
    onehot = (pi == pi.max(axis=1, keepdims=True)).astype(np.float32)
    assert np.array_equal(be.score(x, onehot, z), be.score(x, onehot, z, mask_mode="none"))
    rows = np.full((len(x), 8), SENTINEL, np.float32)
    for bad in (_opts("legal", label_smoothing=1.0), _opts(5), _opts("target", huber_delta=0.0)):
        rc = _lib.lib().m0_net_score(be.handle, _lib.ptr(x), _lib.ptr(pi), _lib.ptr(z), _lib.ptr(mask), len(x), C.byref(bad), _lib.ptr(rows))
        assert _refused(rc, rows)
    good = _opts("legal")
    assert _refused(_lib.lib().m0_net_score(be.handle, _lib.ptr(x), _lib.ptr(pi), _lib.ptr(z), None, len(x), C.byref(good), _lib.ptr(rows)), rows)
    assert _refused(_lib.lib().m0_net_score(be.handle, _lib.ptr(x), None, _lib.ptr(z), _lib.ptr(mask), len(x), C.byref(good), _lib.ptr(rows)), rows)
    assert _refused(_lib.lib().m0_net_score(be.handle, _lib.ptr(x), _lib.ptr(pi), _lib.ptr(z), _lib.ptr(mask), 0, C.byref(good), _lib.ptr(rows)), rows)
    assert _refused(_lib.lib().m0_net_score(None, _lib.ptr(x), _lib.ptr(pi), _lib.ptr(z), _lib.ptr(mask), len(x), C.byref(good), _lib.ptr(rows)), rows)
    with pytest.raises(ValueError):
        be.score(x, pi, z, mask, value_loss="l1")
    with pytest.raises(ValueError):
        be.score(x, pi[:, :100], z, None)


def test_a_poisoned_network_answers_nonfinite_and_still_writes_the_rows(small_net):
    from matrix0_amd.backend import M0Backend, NonFiniteScore
    _, sd, x = small_net
    bad = {k: v.clone() for k, v in sd.items()}
    key = next(k for k, v in bad.items() if v.ndim == 4)
    bad[key].view(-1)[0] = float("nan")
    be = M0Backend.from_state_dict(SMALL, bad)
    try:
        pi, z, mask = _targets(9, len(x))
        rows = np.full((len(x), 8), SENTINEL, np.float32)
        good = _opts("legal")
        rc = _lib.lib().m0_net_score(be.handle, _lib.ptr(x), _lib.ptr(pi), _lib.ptr(z), _lib.ptr(mask), len(x), C.byref(good), _lib.ptr(rows))
        assert rc == _abi.M0_ERR_NONFINITE
        assert ((rows[:, 7].astype(int) & 2) != 0).any() and not (rows == SENTINEL).any() and np.isfinite(rows).all()
        flagged = (rows[:, 7].astype(int) & 2) != 0
        assert not rows[flagged][:, :5].any() and (rows[:, 5] == mask.sum(axis=1)).all()
        with pytest.raises(NonFiniteScore) as e:
            be.score(x, pi, z, mask)
        assert np.array_equal(e.value.rows, rows)
    finally:
        be.close()


# ---- (4) the shard walk with the real backend --------------------------------------------------------------------------------------
def test_score_shards_is_the_sum_of_backend_score_over_its_rows(small_net, tmp_path):
    from matrix0_amd import score as sc
    from matrix0_amd.data_writer import ShardIndex, write_npz
    from tests.test_score import _means, _shard
    be, _, x = small_net
    rng = np.random.default_rng(4)
    shards = [("a_masked.npz", "selfplay", _shard(rng, 6, "masked")), ("b_soft.npz", "selfplay", _shard(rng, 7, "soft"))]
    index = ShardIndex(tmp_path)
    for name, source, d in shards:
        d["s"] = np.ascontiguousarray(np.concatenate([x, x])[: len(d["z"])][::-1])      # real boards, another order
        write_npz(tmp_path / name, d)
        index.add(tmp_path / name, len(d["z"]), source)
    opts = dict(label_smoothing=0.05, value_loss="huber", huber_delta=0.5)
    r = sc.score_shards(tmp_path, be, batch=4, **opts)
    chunk = lambda d, a: be.score(d["s"][a:a + 4], d["pi"][a:a + 4], d["z"][a:a + 4],
                                  d["legal_mask"][a:a + 4] if "legal_mask" in d else None, **opts)
    rows = [np.concatenate([chunk(d, a) for a in range(0, len(d["z"]), 4)]) for _, _, d in shards]
    assert r["rows"] == 13 and r["scored"] == 13 and [v["mask_mode"] for v in r["by_shard"].values()] == ["legal", "target"]
    for key, want in _means(rows, [d["z"] for _, _, d in shards]).items():
        assert r[key] == pytest.approx(want, rel=1e-12, abs=0), key
