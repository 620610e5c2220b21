"""The SSL score on the device: ssl_score_kernel through m0_ssl_score_rows against the host build of the same arithmetic, bit for
bit, and for its determinism; ssl_targets_planes_kernel against ssl_targets_kernel and the reference's golden; m0_net_score_ssl
behind a real forward (M0Backend.score_ssl) on the golden network of tests/golden/ssl_loss.npz; and the argument checks."""
import ctypes as C
import json

import numpy as np
import pytest

from matrix0_amd import _abi, _lib
from tests import ssl_score_cases as cases
from tests import ssl_score_ref as ref
from tests import ssl_score_shim as shim
from tests.golden_ref import load_npz

pytestmark = pytest.mark.gpu

GROUPS = {g["name"]: g for g in cases.groups()}
BATCHES = (1, 5, 67)             # ROWS_PER_WG is 4: one partial workgroup, a whole one and a row, sixteen and three rows
SENTINEL = shim.SENTINEL
TASKS = ref.TASKS


def ssl_score_rows_rc(heads, tasks, planes, targets, B):
    """m0_ssl_score_rows on arrays that may be None: (return code, rows prefilled with SENTINEL)"""
    rows = np.full((max(B, 1), _abi.SSL_SCORE_COLS), SENTINEL, np.float32)
    rc = _lib.lib().m0_ssl_score_rows(0, _lib.ptr(heads), tasks, _lib.ptr(planes), _lib.ptr(targets), B, _lib.ptr(rows))
    return rc, rows


def ssl_score_rows(heads, tasks, planes, targets=None):
    f = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)
    rc, rows = ssl_score_rows_rc(f(heads), tasks, f(planes), f(targets), len(planes))
    assert rc == _abi.M0_OK, _lib.last_error()
    return rows


# ---- (1) the kernel against the host build, and its determinism ---------------------------------------------------------------
@pytest.mark.parametrize("group", GROUPS)
def test_kernel_equals_the_host_build_bit_for_bit_and_a_row_depends_on_itself_alone(group):
    g = GROUPS[group]
    want = shim.score_rows(g["heads"], g["tasks"], g["planes"], g["targets"])
    first = {}                                          # case row -> the bits of its first result
    for B in BATCHES:
        for shift in (0, 3):                            # the same rows at other row indices
            (heads, planes, targets), idx = cases.tiled(g, B, shift)
            got = ssl_score_rows(heads, g["tasks"], planes, targets)
            for b, k in enumerate(idx):
                bits = got[b].tobytes()
                assert bits == want[k].tobytes(), (g["names"][k], B, shift, b, got[b].tolist(), want[k].tolist())
                assert first.setdefault(int(k), bits) == bits
    (heads, planes, targets), _ = cases.tiled(g, 67)
    assert ssl_score_rows(heads, g["tasks"], planes, targets).tobytes() == ssl_score_rows(heads, g["tasks"], planes, targets).tobytes()
    assert len(first) == len(g["names"])


# ---- (2) targets of stored planes ---------------------------------------------------------------------------------------------
def test_targets_of_encoded_planes_equal_the_targets_of_the_positions_and_the_golden():
    from matrix0_amd import encoding as enc, engine as eng
    z = load_npz("ssl_targets.npz")
    fens = [str(f) for f in z["fens"]]
    planes = enc.encode_fens(fens)[0]
    got = eng.ssl_targets_planes(planes)
    want = eng.ssl_targets_fens(fens)
    assert len(fens) == 121 and not got["status"].any()
    for t in TASKS:
        assert got[t].dtype == np.float32 and np.array_equal(got[t], want[t]), t
        assert np.array_equal(got[t], z[t].astype(np.float32)), t
    # unusable rows among usable ones: flagged, and their maps stay as the caller had them
    g = GROUPS["all:planes"]
    p = np.ascontiguousarray(g["planes"], dtype=np.float32)
    out = np.full((len(p), 17, 64), SENTINEL, np.float32)
    status = np.full(len(p), -1, np.int32)
    assert _lib.lib().m0_ssl_targets_planes(0, _lib.ptr(p), len(p), _lib.ptr(out), _lib.ptr(status)) == _abi.M0_OK
    host_out, host_status = shim.targets_planes(p)
    assert np.array_equal(status, host_status) and status.sum() == 4 and np.array_equal(out, host_out)
    assert (out[status == 1] == SENTINEL).all()
    with pytest.raises(ValueError):
        eng.ssl_targets_planes(p[:, :18])


# ---- (3) behind a forward -----------------------------------------------------------------------------------------------------
def _pi_z_mask(B, seed=9):
    rng = np.random.default_rng(seed)
    pi = np.zeros((B, _abi.POLICY_SIZE), np.float32)
    mask = np.zeros((B, _abi.POLICY_SIZE), np.uint8)
    for b in range(B):
        cols = rng.choice(_abi.POLICY_SIZE, size=20 + 7 * b, replace=False)
        mask[b, cols] = 1
        pi[b, cols[:6]] = rng.dirichlet(np.full(6, 0.5)).astype(np.float32)
    return pi, np.array([(-1.0, 0.0, 1.0)[b % 3] for b in range(B)], np.float32), mask


@pytest.fixture(scope="module")
def golden_net():
    from matrix0_amd.backend import M0Backend
    from tests.golden_util import load_net_golden
    from tests.test_ssl_score import golden_targets
    z = load_npz("ssl_loss.npz")
    gold = {k: z[k] for k in z.files}
    cfg, sd, _, _, _, _ = load_net_golden("gn_silu_preact")          # the network the reference computed the losses with
    be = M0Backend.from_state_dict(cfg, sd)
    yield be, cfg, sd, gold["x"].astype(np.float32), golden_targets(gold), json.loads(str(gold["cases_json"]))
    be.close()


def test_backend_score_ssl_is_both_kernels_on_the_forwards_own_outputs(golden_net):
    be, _, _, x, targets, gold_cases = golden_net
    pi, z, mask = _pi_z_mask(len(x))
    opts = dict(label_smoothing=0.05, value_loss="huber", huber_delta=0.5)
    rows, ssl_rows = be.score_ssl(x, pi, z, mask, **opts)
    assert rows.shape == (6, 8) and ssl_rows.shape == (6, 16) and rows.dtype == ssl_rows.dtype == np.float32
    assert be.ssl_tasks == list(TASKS) and not ssl_rows[:, 15].any()
    # the policy and value columns are those of the forward without the heads: the heads only read the trunk
    assert rows.tobytes() == be.score(x, pi, z, mask, **opts).tobytes()
    # the device heads are the forward's
    _, _, heads = be.infer_np_ssl(x)
    heads = np.concatenate([heads[t].reshape(6, -1, 64) for t in TASKS], axis=1)
    assert ssl_rows.tobytes() == ssl_score_rows(heads, 31, x).tobytes(), "the device heads are not the forward's"
    # against the reference module's own numbers, within what the fp16 forward allows (tests/test_ssl_loss.py:78-80)
    c = gold_cases[0]
    mean = dict(zip(TASKS, ssl_rows[:, :5].astype(np.float64).mean(axis=0)))
    print("mean losses", mean, "reference", c["single"])
    assert abs(sum(mean.values()) - c["total"]) <= 2e-3 * c["total"], (mean, c["total"])
    for t, want in c["single"].items():
        assert abs(mean[t] - want) <= 2e-3 * max(1.0, want), (t, mean[t], want)
    # the stored targets of these positions are the planes' own: the same bits, no mismatch
    rows_t, ssl_rows_t = be.score_ssl(x, pi, z, mask, targets, **opts)
    assert rows_t.tobytes() == rows.tobytes() and ssl_rows_t.tobytes() == ssl_rows.tobytes()
    assert be.score_ssl(x, pi, z, mask, targets.reshape(6, 17, 8, 8), **opts)[1].tobytes() == ssl_rows.tobytes()
    # one square altered: that row alone says so, and the other rows keep their bits
    altered = targets.copy()
    altered[3, 16, 20] = -1.0 if altered[3, 16, 20] != -1.0 else 1.0
    got = be.score_ssl(x, pi, z, mask, altered, **opts)[1]
    assert got[:, 15].tolist() == [0, 0, 0, 4, 0, 0] and np.delete(got, 3, axis=0).tobytes() == np.delete(ssl_rows, 3, axis=0).tobytes()
    assert got[3, 4] != ssl_rows[3, 4] and np.array_equal(got[3, :4], ssl_rows[3, :4])
    # the other calls on the handle are what they were
    assert be.score(x, pi, z, mask, **opts).tobytes() == rows.tobytes()
    with pytest.raises(ValueError):
        be.score_ssl(x, pi, z, mask, targets[:, :16])


def test_score_arrays_with_ssl_chunks_through_the_backend(golden_net):
    from matrix0_amd import score as sc
    be, _, _, x, targets, _ = golden_net
    pi, z, mask = _pi_z_mask(len(x))
    whole = be.score_ssl(x, pi, z, mask, targets)
    rows, ssl_rows = sc.score_arrays(be, x, pi, z, mask, batch=4, ssl="auto", ssl_targets=targets)
    assert rows.tobytes() == whole[0].tobytes() and ssl_rows.tobytes() == whole[1].tobytes()
    assert sc.score_arrays(be, x, pi, z, mask, batch=4, ssl="planes", ssl_targets=targets)[1].tobytes() == whole[1].tobytes()


def _net_score_ssl_rc(handle, x, pi, z, mask, targets, B):
    n = next(len(a) for a in (x, pi, z) if a is not None)
    rows = np.full((n, 8), SENTINEL, np.float32)
    ssl_rows = np.full((n, 16), SENTINEL, np.float32)
    opts = _abi.ScoreOpts(_abi.SCORE_MASK["legal"], 0.0, 0, 1.0)
    rc = _lib.lib().m0_net_score_ssl(handle, _lib.ptr(x), _lib.ptr(pi), _lib.ptr(z), _lib.ptr(mask), _lib.ptr(targets), B,
                                     C.byref(opts), _lib.ptr(rows), _lib.ptr(ssl_rows))
    return rc, rows, ssl_rows


def test_a_network_without_ssl_heads_is_refused():
    from matrix0_amd.backend import M0Backend
    from tests import net_layer_cases as net_cases
    from tests.test_score_gpu import SMALL
    be = M0Backend.from_state_dict(SMALL, net_cases.weights(SMALL, sharp=True))
    try:
        x = net_cases.planes().numpy().astype(np.float32)
        pi, z, mask = _pi_z_mask(len(x))
        rc, rows, ssl_rows = _net_score_ssl_rc(be.handle, x, pi, z, mask, None, len(x))
        assert rc == _abi.M0_ERR_INVALID and (rows == SENTINEL).all() and (ssl_rows == SENTINEL).all()
        with pytest.raises(ValueError):
            be.score_ssl(x, pi, z, mask)
        assert be.ssl_tasks == []
    finally:
        be.close()


def test_a_poisoned_head_answers_nonfinite_and_still_writes_both_arrays(golden_net):
    from matrix0_amd.backend import M0Backend, NonFiniteScore
    _, cfg, sd, x, _, _ = golden_net
    bad = {k: v.clone() for k, v in sd.items()}
    bad["ssl_heads.fork.3.weight"].view(-1)[0] = float("nan")
    be = M0Backend.from_state_dict(cfg, bad)
    try:
        pi, z, mask = _pi_z_mask(len(x))
        rc, rows, ssl_rows = _net_score_ssl_rc(be.handle, x, pi, z, mask, None, len(x))
        assert rc == _abi.M0_ERR_NONFINITE
        assert not (rows == SENTINEL).any() and not (ssl_rows == SENTINEL).any() and np.isfinite(rows).all() and np.isfinite(ssl_rows).all()
        flagged = (ssl_rows[:, 15].astype(int) & 2) != 0
        assert flagged.any() and not ssl_rows[flagged][:, :15].any()
        assert not (rows[:, 7].astype(int) & 2).any() and (rows[:, 0] > 0).all()        # policy and value do not pass the head
        with pytest.raises(NonFiniteScore) as e:
            be.score_ssl(x, pi, z, mask)
        assert np.array_equal(e.value.rows, rows) and np.array_equal(e.value.ssl_rows, ssl_rows)
    finally:
        be.close()


# ---- (4) argument checks ------------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused_and_touch_nothing(golden_net):
    (heads, planes, targets), _ = cases.tiled(GROUPS["all:stored"], 3)
    refused = lambda rc, *outs: rc == _abi.M0_ERR_INVALID and all((o == SENTINEL).all() for o in outs)
    assert ssl_score_rows_rc(heads, 31, planes, targets, 3)[0] == _abi.M0_OK
    assert ssl_score_rows_rc(heads, 31, planes, None, 3)[0] == _abi.M0_OK
    assert _lib.lib().m0_ssl_score_rows(0, _lib.ptr(heads), 31, _lib.ptr(planes), None, 3, None) == _abi.M0_ERR_INVALID
    assert refused(*ssl_score_rows_rc(None, 31, planes, targets, 3)) and refused(*ssl_score_rows_rc(heads, 31, None, targets, 3))
    for B in (0, -1):
        assert refused(*ssl_score_rows_rc(heads, 31, planes, targets, B)), B
    for tasks in (0, 32, 63, -1):
        assert refused(*ssl_score_rows_rc(heads, tasks, planes, targets, 3)), tasks
    out = np.full((3, 17, 64), SENTINEL, np.float32)
    status = np.full(3, -1, np.int32)
    L = _lib.lib()
    for args in ((None, 3, _lib.ptr(out), _lib.ptr(status)), (_lib.ptr(planes), 0, _lib.ptr(out), _lib.ptr(status)),
                 (_lib.ptr(planes), 3, None, _lib.ptr(status)), (_lib.ptr(planes), 3, _lib.ptr(out), None)):
        assert L.m0_ssl_targets_planes(0, *args) == _abi.M0_ERR_INVALID
    assert (out == SENTINEL).all() and (status == -1).all()
    us, nbytes = C.c_float(-1), C.c_double(-1)
    for B, tasks, iters in ((0, 31, 1), (4, 0, 1), (4, 31, 0), (4, 64, 1)):
        assert L.m0_ssl_score_bench(0, B, tasks, 1, iters, C.byref(us), C.byref(nbytes)) == _abi.M0_ERR_INVALID
    assert L.m0_ssl_score_bench(0, 4, 31, 1, 1, None, C.byref(nbytes)) == _abi.M0_ERR_INVALID and us.value == -1 and nbytes.value == -1
    assert L.m0_ssl_score_bench(0, 5, 31, 0, 2, C.byref(us), C.byref(nbytes)) == _abi.M0_OK
    assert us.value > 0 and nbytes.value == 5 * (19 * 256 + 13 * 256 + 17 * 256 + 64)
    assert L.m0_ssl_score_bench(0, 5, 17, 1, 2, C.byref(us), C.byref(nbytes)) == _abi.M0_OK and nbytes.value == 5 * (16 * 256 + 13 * 256 + 64)
    # behind the forward: what m0_net_score refuses, and a null ssl_rows
    be, _, _, x, tg, _ = golden_net
    pi, z, mask = _pi_z_mask(len(x))
    assert _net_score_ssl_rc(be.handle, x, pi, z, mask, tg, len(x))[0] == _abi.M0_OK
    for k in range(3):
        args = [x, pi, z]
        args[k] = None
        assert refused(*_net_score_ssl_rc(be.handle, *args, mask, tg, len(x))), k
    assert refused(*_net_score_ssl_rc(be.handle, x, pi, z, None, tg, len(x))), "legal without a mask"
    assert refused(*_net_score_ssl_rc(be.handle, x, pi, z, mask, tg, 0)) and refused(*_net_score_ssl_rc(None, x, pi, z, mask, tg, len(x)))
    rows = np.full((len(x), 8), SENTINEL, np.float32)
    opts = _abi.ScoreOpts(_abi.SCORE_MASK["legal"], 1.5, 0, 1.0)
    for o, r in ((opts, _lib.ptr(rows)), (_abi.ScoreOpts(0, 0.0, 0, 1.0), None)):
        assert L.m0_net_score_ssl(be.handle, _lib.ptr(x), _lib.ptr(pi), _lib.ptr(z), _lib.ptr(mask), None, len(x), C.byref(o),
                                  _lib.ptr(rows), r) == _abi.M0_ERR_INVALID
    assert (rows == SENTINEL).all()
