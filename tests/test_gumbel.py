"""The Gumbel root search without a GPU: the host exports of csrc/gumbel_core.h (m0_gumbel_schedule, m0_gumbel_improve) against
tests/gumbel_ref.py, the `mcts.gumbel` block of the configuration, and what the setter refuses before it needs an engine."""
import ctypes as C

import numpy as np
import pytest

from matrix0_amd import _abi, _lib, engine as eng
from tests import gumbel_ref as gr

M_EFF = [1, 2, 3, 4, 5, 8, 16, 17, 64, 200]
SIMS = list(range(1, 71)) + [200, 800]


@pytest.mark.parametrize("m_eff", M_EFF)
def test_schedule_equals_the_reference(m_eff):
    for n in SIMS:
        seq, end = eng.gumbel_schedule(m_eff, n)
        want_seq, want_end = gr.considered_visits(m_eff, n)
        assert seq.tolist() == want_seq, (m_eff, n)
        assert end.tolist() == want_end, (m_eff, n)
        assert all(s < e <= n for s, e in enumerate(end.tolist()))


@pytest.mark.parametrize("m_eff", M_EFF)
def test_every_scheduled_visit_finds_a_candidate_of_its_own(m_eff):
    """Simulation s asks for a child with seq[s] visits: with the counts simulated, m_eff children starting at 0 and the one
    taken always among the first `considered`, there always is one, and no phase hands a child two visits at the same count."""
    for n in SIMS:
        seq, end = eng.gumbel_schedule(m_eff, n)
        cnt = [0] * max(1, m_eff)
        s = 0
        while s < n:
            taken = set()
            for t in range(s, int(end[s])):
                cand = [i for i in range(len(cnt)) if cnt[i] == seq[t]]
                assert cand, (m_eff, n, t)
                i = cand[0]                                  # any fixed order of preference: the lowest index
                assert (i, int(seq[t])) not in taken
                taken.add((i, int(seq[t])))
                cnt[i] += 1
            s = int(end[s])
        assert sum(cnt) == n


def test_schedule_arguments():
    L = _lib.lib()
    assert L.m0_gumbel_schedule(-1, 4, None, None) == _lib.M0_ERR_INVALID
    assert L.m0_gumbel_schedule(4, -1, None, None) == _lib.M0_ERR_INVALID
    assert L.m0_gumbel_schedule(4, 0, None, None) == _lib.M0_OK
    seq = np.zeros(8, np.int32)
    assert L.m0_gumbel_schedule(4, 8, _lib.ptr(seq), None) == _lib.M0_OK and seq.tolist() == gr.considered_visits(4, 8)[0]


def _random_root(rng, k, visited):
    """prior (float32 values summing to 1, as the engine stores them), q, n, gl, root_v; `visited` in {"none", "all", "some"}"""
    prior = rng.dirichlet(np.full(k, 0.5)).astype(np.float32).astype(np.float64)
    prior = np.maximum(prior, 1e-12)
    q = rng.uniform(-1.0, 1.0, k)
    if visited == "none":
        n = np.zeros(k, np.int32)
    elif visited == "all":
        n = rng.integers(1, 9, k).astype(np.int32)
    else:
        n = (rng.integers(0, 6, k) * (rng.random(k) < 0.5)).astype(np.int32)
    q = np.where(n > 0, q, 0.0)
    gl = -np.log(-np.log(rng.random(k))) + np.log(prior)
    return prior, q, n, gl, float(rng.uniform(-1.0, 1.0))


@pytest.mark.parametrize("k", [1, 2, 3, 20, 64, 65, 218])
@pytest.mark.parametrize("visited", ["none", "all", "some"])
def test_improve_equals_the_reference(k, visited):
    rng = np.random.default_rng(1000 * k + len(visited))
    for c_visit, c_scale in [(50.0, 1.0), (50.0, 0.1), (0.0, 1.0), (10.0, 0.0)]:
        for _ in range(8):
            prior, q, n, gl, root_v = _random_root(rng, k, visited)
            pi, v_mix, pick = eng.gumbel_improve(prior, q, n, gl, root_v, c_visit, c_scale)
            want_pi, want_v, want_pick, gap = gr.improve(prior, q, n, gl, root_v, c_visit, c_scale)
            np.testing.assert_allclose(pi, want_pi, rtol=0, atol=1e-12)
            assert abs(v_mix - want_v) <= 1e-12
            assert abs(pi.sum() - 1.0) <= 1e-12 and np.all(pi > 0)
            if visited == "none":
                assert v_mix == root_v
            assert gap > 1e-9, "a seeded case with two best moves: the pick would hang on the last bit"
            assert pick == want_pick


def test_improve_takes_the_lowest_index_among_equal_children():
    prior = np.full(4, 0.25)
    pi, v_mix, pick = eng.gumbel_improve(prior, np.zeros(4), np.array([2, 3, 3, 1]), np.array([5.0, 1.0, 1.0, 9.0]), 0.0)
    assert pick == 1                                       # most visits first, then the score, then the index
    np.testing.assert_allclose(pi, gr.improve(prior, np.zeros(4), [2, 3, 3, 1], [5.0, 1.0, 1.0, 9.0], 0.0)[0], atol=1e-12)
    assert eng.gumbel_improve(prior, np.zeros(4), np.array([3, 3, 3, 1]), np.array([0.0, 2.0, 1.0, 9.0]), 0.0)[2] == 1


def test_improve_arguments():
    L = _lib.lib()
    a, n = np.full(3, 1 / 3), np.zeros(3, np.int32)
    ok = _abi.GumbelCfg(16, 50.0, 1.0)

    def call(k, cfg, prior=a):
        return L.m0_gumbel_improve(k, _lib.ptr(prior), _lib.ptr(a), _lib.ptr(n), _lib.ptr(a), 0.0, cfg, None, None, None)

    assert call(3, C.byref(ok)) == _lib.M0_OK
    assert call(0, C.byref(ok)) == call(257, C.byref(ok)) == call(3, None) == call(3, C.byref(ok), prior=None) == _lib.M0_ERR_INVALID
    for bad in [(16, -1.0, 1.0), (16, 50.0, -0.5), (16, float("nan"), 1.0), (16, 50.0, float("inf"))]:
        assert call(3, C.byref(_abi.GumbelCfg(*bad))) == _lib.M0_ERR_INVALID, bad


def test_the_setter_and_the_result_refuse_a_null_engine():
    L = _lib.lib()
    ok = _abi.GumbelCfg(16, 50.0, 1.0)
    assert L.m0_selfplay_set_gumbel(None, C.byref(ok)) == _lib.M0_ERR_INVALID
    assert L.m0_search_gumbel_result(None, 0, None, None, None, None, None) == _lib.M0_ERR_INVALID


def test_config_block():
    assert eng.gumbel_cfg_from_dict({}) is None and eng.gumbel_cfg_from_dict({"mcts": {"cpuct": 2.0}}) is None
    assert eng.gumbel_cfg_from_dict({"mcts": {"gumbel": None}}) is None
    assert eng.gumbel_cfg_from_dict({"mcts": {"gumbel": {"enabled": False}}}) is None
    g = eng.gumbel_cfg_from_dict({"mcts": {"gumbel": {"enabled": True}}})
    assert (g.max_considered, g.c_visit, g.c_scale) == (16, 50.0, 1.0)            # the paper's constants
    g = eng.gumbel_cfg_from_dict({"mcts": {"gumbel": {"enabled": True, "max_considered": 4, "c_visit": 25, "c_scale": 0.5}}})
    assert (g.max_considered, g.c_visit, g.c_scale) == (4, 25.0, 0.5)
    # the PUCT configuration does not see the block
    base = {"mcts": {"cpuct": 2.0}, "selfplay": {"num_simulations": 16}}
    with_block = {"mcts": {"cpuct": 2.0, "gumbel": {"enabled": True}}, "selfplay": {"num_simulations": 16}}
    assert bytes(eng.selfplay_cfg_from_dict(base, concurrent_games=2)) == bytes(eng.selfplay_cfg_from_dict(with_block, concurrent_games=2))


@pytest.mark.parametrize("block", [True, "on", 16, [], {}, {"max_considered": 16}, {"enabled": 1}, {"enabled": "yes"},
                                   {"enabled": True, "max_considered": 0}, {"enabled": True, "max_considered": 257},
                                   {"enabled": True, "max_considered": 16.0}, {"enabled": True, "max_considered": True},
                                   {"enabled": False, "max_considered": -3}, {"enabled": True, "c_visit": -1.0},
                                   {"enabled": True, "c_scale": float("nan")}, {"enabled": True, "c_visit": float("inf")},
                                   {"enabled": True, "c_scale": "1"}, {"enabled": True, "considered": 8}])
def test_a_malformed_config_block_is_an_error(block):
    with pytest.raises(ValueError, match="gumbel"):
        eng.gumbel_cfg_from_dict({"mcts": {"gumbel": block}})


def test_the_config_block_refuses_the_position_table():
    cfg = {"mcts": {"gumbel": {"enabled": True}}, "engine": {"compat": {"tt_merge": True}}}
    with pytest.raises(ValueError, match="tt_merge"):
        eng.gumbel_cfg_from_dict(cfg)
