"""The self-play budget mix without a GPU (include/m0_budget.h): the three host calls against tests/budget_ref.py, hand cases of the
pruning, the config parser's refusals and the worker's row filter on fake records."""
import ctypes as C
import glob
import math
import os

import numpy as np
import pytest

from matrix0_amd import _abi, _lib, engine as eng
from oracle import mcts_ref as ref
from tests import budget_ref as br


def _random_root(rng):
    """k children (1 .. 218) with priors that sum to 1, values in [-1, 1] and up to 1 600 visits spread unevenly; some roots
    carry many unvisited children, some a few visits only."""
    k = int(rng.integers(1, 219))
    prior = rng.dirichlet(np.full(k, float(rng.choice([0.05, 0.3, 1.0]))))
    prior = np.clip(prior, 1e-8, 1.0 - 1e-8)
    q = rng.uniform(-1.0, 1.0, k)
    total = int(rng.integers(0, 1601))
    share = rng.dirichlet(np.full(k, float(rng.choice([0.05, 0.5])))) if total else np.zeros(k)
    n = np.floor(share * total).astype(np.int32)
    root_n = int(n.sum()) + int(rng.integers(0, 3))
    cpuct = float(rng.uniform(1.0, 3.5))
    forced_k = float(rng.choice([0.0, 0.5, 2.0, 4.0]))
    return prior, q, n, root_n, cpuct, forced_k


def test_prune_equals_the_reference_on_random_roots():
    rng = np.random.default_rng(20240607)
    changed = 0
    for case in range(1000):
        prior, q, n, root_n, cpuct, forced_k = _random_root(rng)
        pn, pi, best = eng.budget_prune(prior, q, n, root_n, cpuct, forced_k)
        want_n, want_pi, want_best, _ = br.prune(prior, q, n, root_n, cpuct, forced_k)
        assert pn.tolist() == want_n.tolist(), case
        assert best == want_best, case
        np.testing.assert_allclose(pi, want_pi, rtol=0, atol=1e-15)
        assert np.all(pn <= n) and np.all(pn >= 0)
        if n.sum() > 0:
            assert pn[best] == n[best] and abs(pi.sum() - 1.0) <= 1e-12
        changed += int(np.any(pn != n))
    assert changed > 100, "the random roots hardly ever had a visit to prune"


def test_forced_and_is_full_equal_the_reference():
    rng = np.random.default_rng(7)
    for _ in range(1000):
        k, p, n = float(rng.uniform(0.0, 4.0)), float(rng.uniform(0.0, 1.0)), int(rng.integers(0, 1601))
        assert eng.budget_forced(k, p, n) == br.n_forced(k, p, n)
    assert eng.budget_forced(2.0, 0.5, 100) == 10.0 and eng.budget_forced(0.0, 0.5, 100) == 0.0
    for seed, game in [(1234, 0), (77, 5), (2 ** 63 + 11, 1 << 20)]:
        for p in (0.25, 0.5, 1.0):
            got = [eng.budget_is_full(seed, game, ply, p) for ply in range(64)]
            assert got == [br.is_full(seed, game, ply, p) for ply in range(64)]
            assert all(got) if p == 1.0 else (any(got) and not all(got))
    # the stream is the game's own: neither another game's nor the game stream's draws
    s = ref.Stream(ref.derive_seed(1234, 0, br.PURPOSE_BUDGET))
    assert [eng.budget_is_full(1234, 0, ply, 0.5) for ply in range(32)] == [s.next() < 0.5 for _ in range(32)]
    assert br.PURPOSE_BUDGET == 7 and br.PURPOSE_BUDGET not in (ref.PURPOSE_JITTER, ref.PURPOSE_NOISE, ref.PURPOSE_DIRICHLET,
                                                                 ref.PURPOSE_GAME)


def test_prune_hand_cases():
    # a single child
    pn, pi, best = eng.budget_prune([1.0], [0.3], [17], 17, 2.5, 2.0)
    assert pn.tolist() == [17] and pi.tolist() == [1.0] and best == 0
    # all visits on one child: nothing else has a visit to lose
    pn, pi, best = eng.budget_prune([0.5, 0.3, 0.2], [0.1, 0.0, 0.0], [0, 40, 0], 40, 2.5, 2.0)
    assert pn.tolist() == [0, 40, 0] and pi.tolist() == [0.0, 1.0, 0.0] and best == 1
    # no visit at all
    pn, pi, best = eng.budget_prune([0.5, 0.5], [0.0, 0.0], [0, 0], 0, 2.5, 2.0)
    assert pn.tolist() == [0, 0] and pi.tolist() == [0.0, 0.0] and best == -1
    # a child with n = 1 whose only visit the forcing may have brought: 1 -> 0 is the range [0, 1], and 0 is below S only if
    # its PUCT value without a visit is; here it is not, so it keeps its visit
    prior, q, n = [0.6, 0.4], [0.5, 0.9], [99, 1]
    pn, _, best = eng.budget_prune(prior, q, n, 100, 2.5, 2.0)
    assert best == 0 and pn.tolist() == br.prune(prior, q, n, 100, 2.5, 2.0)[0].tolist() == [99, 1]
    # ... and with a poor value it goes: PUCT(1; 0) = -0.9 + 2.5 * 0.01 * 10 = -0.65 < S
    prior, q, n = [0.99, 0.01], [0.5, -0.9], [99, 1]
    pn, pi, _ = eng.budget_prune(prior, q, n, 100, 2.5, 2.0)
    assert pn.tolist() == [99, 0] and pi.tolist() == [1.0, 0.0]
    # a child reduced to exactly 1 of more becomes 0: n = 3, F = ceil(sqrt(2 * 0.02 * 100)) = 2, range [1, 3], below S at 1
    prior, q, n = [0.98, 0.02], [0.5, -0.9], [97, 3]
    assert math.ceil(br.n_forced(2.0, 0.02, 100)) == 2
    pn, _, _ = eng.budget_prune(prior, q, n, 100, 2.5, 2.0)
    assert pn.tolist() == br.prune(prior, q, n, 100, 2.5, 2.0)[0].tolist() == [97, 0]
    # forced_k = 0 is the identity
    rng = np.random.default_rng(3)
    for _ in range(20):
        prior, q, n, root_n, cpuct, _ = _random_root(rng)
        pn, pi, _ = eng.budget_prune(prior, q, n, root_n, cpuct, 0.0)
        assert pn.tolist() == n.tolist()
        if n.sum():
            np.testing.assert_allclose(pi, n / n.sum(), rtol=0, atol=1e-15)
    # the most visited child is not the PUCT maximum: every other child's value at its full count is already above S, no
    # count in its range is below it, and nothing is subtracted
    prior, q, n = [0.2, 0.4, 0.4], [-0.8, 0.6, 0.5], [50, 30, 20]
    sq = math.sqrt(100.0)
    S = br.puct(q[0], 2.5, prior[0], sq, 50)
    assert all(br.puct(q[i], 2.5, prior[i], sq, n[i]) > S for i in (1, 2))
    pn, pi, best = eng.budget_prune(prior, q, n, 100, 2.5, 2.0)
    assert best == 0 and pn.tolist() == [50, 30, 20] and pi.tolist() == [0.5, 0.3, 0.2]
    # the most visited child, lowest index among equals
    assert eng.budget_prune([0.3, 0.3, 0.4], [0.0, 0.0, 0.0], [5, 9, 9], 23, 2.5, 2.0)[2] == 1


def test_arguments_of_the_host_calls():
    L = _lib.lib()
    a, n = np.full(3, 1 / 3), np.ones(3, np.int32)
    full, out = C.c_int(0), C.c_double(0)

    def prune(k, prior=a, q=a, nn=n, forced_k=2.0):
        return L.m0_budget_prune(k, _lib.ptr(prior), _lib.ptr(q), _lib.ptr(nn), 3, 2.5, forced_k, None, None, None)

    assert prune(3) == _lib.M0_OK
    assert prune(0) == prune(257) == prune(3, prior=None) == prune(3, q=None) == prune(3, nn=None) == _lib.M0_ERR_INVALID
    assert prune(3, forced_k=-1.0) == prune(3, forced_k=float("nan")) == prune(3, forced_k=float("inf")) == _lib.M0_ERR_INVALID
    assert prune(3, nn=np.array([1, -1, 1], np.int32)) == _lib.M0_ERR_INVALID
    assert L.m0_budget_is_full(1, 0, 0, 0.5, C.byref(full)) == _lib.M0_OK
    for bad in [(1, 0, -1, 0.5), (1, 0, 0, 0.0), (1, 0, 0, 1.5), (1, 0, 0, float("nan"))]:
        assert L.m0_budget_is_full(*bad, C.byref(full)) == _lib.M0_ERR_INVALID, bad
    assert L.m0_budget_is_full(1, 0, 0, 0.5, None) == _lib.M0_ERR_INVALID
    assert L.m0_budget_forced(2.0, 0.5, 10, C.byref(out)) == _lib.M0_OK
    for bad in [(-1.0, 0.5, 10), (2.0, -0.5, 10), (2.0, 0.5, -1), (float("inf"), 0.5, 10), (2.0, float("nan"), 10)]:
        assert L.m0_budget_forced(*bad, C.byref(out)) == _lib.M0_ERR_INVALID, bad
    assert L.m0_budget_forced(2.0, 0.5, 10, None) == _lib.M0_ERR_INVALID
    # the engine calls refuse a null engine
    ok = _abi.BudgetCfg(0.25, 100, 2.0, 1)
    assert L.m0_selfplay_set_budget(None, C.byref(ok)) == _lib.M0_ERR_INVALID
    assert L.m0_search_budget_result(None, 0, None, None, None) == _lib.M0_ERR_INVALID
    assert L.m0_selfplay_budget_stats(None, None) == _lib.M0_ERR_INVALID
    assert L.m0_game_record_budget(None, None, None) == _lib.M0_ERR_INVALID
    # a record without an owner is a record of an engine without the mode
    rec = _abi.GameRecord()
    f, s = C.POINTER(C.c_uint8)(), C.POINTER(C.c_int)()
    assert L.m0_game_record_budget(C.byref(rec), C.byref(f), C.byref(s)) == _lib.M0_OK and not f and not s


def test_config_block():
    assert eng.budget_cfg_from_dict({}) is None and eng.budget_cfg_from_dict({"mcts": {"cpuct": 2.0}}) is None
    assert eng.budget_cfg_from_dict({"mcts": {"budget": None}}) is None
    assert eng.budget_cfg_from_dict({"mcts": {"budget": {"enabled": False}}}) is None
    b = eng.budget_cfg_from_dict({"mcts": {"budget": {"enabled": True}}})
    assert (b.full_prob, b.fast_simulations, b.forced_k, b.prune_targets) == (0.25, 100, 2.0, 1)
    b = eng.budget_cfg_from_dict({"mcts": {"budget": {"enabled": True, "full_prob": 1, "fast_simulations": 12, "forced_k": 0,
                                                      "prune_targets": False}}})
    assert (b.full_prob, b.fast_simulations, b.forced_k, b.prune_targets) == (1.0, 12, 0.0, 0)
    # the engine's configuration does not see the block
    base = {"mcts": {"cpuct": 2.0}, "selfplay": {"num_simulations": 16}}
    with_block = {"mcts": {"cpuct": 2.0, "budget": {"enabled": True}}, "selfplay": {"num_simulations": 16}}
    assert bytes(eng.selfplay_cfg_from_dict(base, concurrent_games=2)) == bytes(eng.selfplay_cfg_from_dict(with_block, concurrent_games=2))
    # a disabled Gumbel block beside it is no conflict
    assert eng.budget_cfg_from_dict({"mcts": {"budget": {"enabled": True}, "gumbel": {"enabled": False}}}) is not None


@pytest.mark.parametrize("block", [True, "on", 16, [], {}, {"full_prob": 0.5}, {"enabled": 1}, {"enabled": "yes"},
                                   {"enabled": True, "full_prob": 0}, {"enabled": True, "full_prob": 1.5},
                                   {"enabled": True, "full_prob": "0.5"}, {"enabled": True, "full_prob": True},
                                   {"enabled": True, "full_prob": float("nan")}, {"enabled": True, "fast_simulations": 0},
                                   {"enabled": True, "fast_simulations": 100.0}, {"enabled": True, "fast_simulations": True},
                                   {"enabled": False, "fast_simulations": -3}, {"enabled": True, "forced_k": -1.0},
                                   {"enabled": True, "forced_k": float("nan")}, {"enabled": True, "forced_k": float("inf")},
                                   {"enabled": True, "forced_k": "2"}, {"enabled": True, "prune_targets": 1},
                                   {"enabled": True, "prune_targets": "yes"}, {"enabled": True, "fast_sims": 8}])
def test_a_malformed_config_block_is_an_error(block):
    with pytest.raises(ValueError, match="budget"):
        eng.budget_cfg_from_dict({"mcts": {"budget": block}})


@pytest.mark.parametrize("other,word", [({"mcts": {"gumbel": {"enabled": True}}}, "gumbel"),
                                        ({"engine": {"proof_search": True}}, "proof_search"),
                                        ({"engine": {"compat": {"tt_merge": True}}}, "tt_merge")])
def test_the_config_block_refuses_the_other_modes(other, word):
    cfg = {"mcts": dict({"budget": {"enabled": True}}, **other.get("mcts", {})), "engine": other.get("engine", {})}
    with pytest.raises(ValueError, match=word):
        eng.budget_cfg_from_dict(cfg)
    cfg["mcts"]["budget"] = {"enabled": False}
    assert eng.budget_cfg_from_dict(cfg) is None


# ---- the worker's row filter, on an engine that hands out fake records

def _fake_record(game_index, full, ssl):
    T = len(full)
    rng = np.random.default_rng(100 + game_index)
    rec = {"game_index": game_index, "moves": T, "resigned": False, "resigner": None, "draw": False, "result": 1.0,
           "avg_policy_entropy": 1.5, "avg_sims": 40.0, "secs": 0.5, "played": ["e2e4"] * T,
           "s": rng.random((T, 19, 8, 8), dtype=np.float32), "pi": rng.random((T, 4672), dtype=np.float32),
           "legal_mask": (rng.random((T, 4672)) < 0.01).astype(np.uint8),
           "z": np.where(np.arange(T) % 2 == 0, 1.0, -1.0).astype(np.float32), "search_values": np.zeros(T, np.float32),
           "full": np.array(full, bool), "sims": np.where(np.array(full, bool), 48, 12).astype(np.int32)}
    if ssl:
        rec["ssl"] = {"piece": rng.random((T, 13, 8, 8), dtype=np.float32), "control": rng.random((T, 8, 8), dtype=np.float32)}
    return rec


class _FakeEngine:
    made = []

    def __init__(self, backend, cfg):
        self.records = list(_FakeEngine.queue)
        self.budget = None
        _FakeEngine.made.append(self)

    def set_budget(self, b):
        self.budget = b

    def running(self):
        return bool(self.records)

    def step(self, steps=1):
        pass

    def poll(self):
        return self.records.pop(0) if self.records else None

    def stats(self):
        return {"arena_overflows": 0, "plies": 0, "sims": 0, "ssl_dropped": 0}

    def close(self):
        pass


class _FakeBackend:
    @classmethod
    def from_state_dict(cls, *a, **k):
        return cls()

    from_checkpoint = from_state_dict

    def close(self):
        pass


class _Queue(list):
    put = list.append


def _run_worker(monkeypatch, tmp_path, records, replay=False, ssl=False):
    from matrix0_amd import selfplay as spw
    _FakeEngine.queue, _FakeEngine.made = records, []
    monkeypatch.setattr(spw, "SelfplayEngine", _FakeEngine)
    monkeypatch.setattr(spw, "M0Backend", _FakeBackend)
    monkeypatch.setattr(spw, "random_state_dict", lambda *a, **k: {})
    monkeypatch.setattr(spw, "detect_value_from_white", lambda be: False)
    monkeypatch.setattr(_lib, "device_count", lambda: 1)
    model = {"channels": 64, "self_supervised": ssl, "ssl_tasks": ["piece", "control"]}
    cfg = {"seed": 5, "model": model, "data_dir": str(tmp_path), "selfplay": {"num_simulations": 48},
           "mcts": {"budget": {"enabled": True, "full_prob": 0.5, "fast_simulations": 12}},
           "engine": {"concurrent_games": 2, "replay_shards": replay}}
    q = _Queue()
    spw.selfplay_worker(0, cfg, None, len(records), q)
    assert len(_FakeEngine.made) == 1 and _FakeEngine.made[0].budget.fast_simulations == 12
    return q


def test_the_worker_writes_the_full_rows_in_order_and_nothing_for_a_game_without_one(monkeypatch, tmp_path):
    full = [True, False, False, True, True, False, True]
    recs = [_fake_record(0, full, True), _fake_record(1, [False] * 5, True), _fake_record(2, [True] * 3, True)]
    want = [{k: (dict(v) if isinstance(v, dict) else v) for k, v in r.items()} for r in recs]
    q = _run_worker(monkeypatch, tmp_path, recs, ssl=True)
    games = [m for m in q if m["type"] == "game"]
    assert [m["moves"] for m in games] == [7, 5, 3]                 # plies played, as ever
    assert games[1]["file"] is None and games[0]["file"] and games[2]["file"]
    files = sorted(glob.glob(os.path.join(str(tmp_path), "selfplay", "*.npz")))
    assert sorted([games[0]["file"], games[2]["file"]]) == files     # the game without a full search wrote nothing
    for g, rec in ((games[0], want[0]), (games[2], want[2])):
        keep = rec["full"]
        with np.load(g["file"]) as d:
            for key in ("s", "pi", "z", "legal_mask"):
                assert np.array_equal(d[key], rec[key][keep]), key
            assert np.array_equal(d["ssl_piece"], rec["ssl"]["piece"][keep])
            assert np.array_equal(d["ssl_control"], rec["ssl"]["control"][keep])
            assert d["meta_plies"].tolist() == [len(keep)] and d["meta_full_rows"].tolist() == [int(keep.sum())]
            assert d["meta_moves"].tolist() == [len(keep)]
            rows = {key: d[key].shape[0] for key in d.files if not key.startswith("meta_")}
            assert set(rows.values()) == {int(keep.sum())}, rows


@pytest.mark.parametrize("replay", [True, "packed"])
def test_the_replay_writers_get_the_same_filtered_rows(monkeypatch, tmp_path, replay):
    from matrix0_amd import selfplay as spw
    seen = []
    real = spw.ReplayShardWriter.add_game

    def add_game(self, data):
        seen.append({k: np.array(v) for k, v in data.items()})
        return real(self, data)

    monkeypatch.setattr(spw.ReplayShardWriter, "add_game", add_game)
    full = [False, True, True, False]
    recs = [_fake_record(0, full, False), _fake_record(1, [False, False], False)]
    want = {k: np.array(v) for k, v in recs[0].items() if isinstance(v, np.ndarray)}
    q = _run_worker(monkeypatch, tmp_path, recs, replay=replay)
    assert [m["moves"] for m in q if m["type"] == "game"] == [4, 2]
    assert len(seen) == 1                                            # the second game has no full ply
    keep = want["full"]
    for key in ("s", "pi", "z", "legal_mask"):
        assert np.array_equal(seen[0][key], want[key][keep]), key
    assert seen[0]["meta_plies"].tolist() == [4] and seen[0]["meta_full_rows"].tolist() == [2]
    assert len(glob.glob(os.path.join(str(tmp_path), "replays", "*.npz"))) == 1


def test_keep_full_rows_leaves_the_metadata_alone():
    from matrix0_amd.selfplay import keep_full_rows
    data = {"s": np.arange(3 * 19 * 64, dtype=np.float32).reshape(3, 19, 8, 8), "z": np.array([1, -1, 1], np.float32),
            "meta_moves": np.array([3], np.int32), "meta_result": np.array([1.0], np.float32)}
    out = keep_full_rows(data, [False, True, False])
    assert out["s"].shape == (1, 19, 8, 8) and np.array_equal(out["s"][0], data["s"][1]) and out["z"].tolist() == [-1.0]
    assert out["meta_moves"].tolist() == [3] and out["meta_plies"].tolist() == [3] and out["meta_full_rows"].tolist() == [1]
    one = keep_full_rows({"s": data["s"][:1], "z": data["z"][:1], "meta_moves": np.array([1], np.int32)}, [True])
    assert one["meta_moves"].tolist() == [1] and one["s"].shape[0] == 1
