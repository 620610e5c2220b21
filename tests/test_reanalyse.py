"""Host side of reanalyse (no GPU): the target rule, every reason a row keeps its targets, ids over shard boundaries and the
shard tool, against a stand-in engine behind the real Analyzer (in the manner of tests/test_analysis.py).  The stand-in
decodes with the host build of the planes decode (tests/host_shim/planes_shim.cpp) and answers each row with visit counts drawn from its
id alone, so that a result can only depend on what the real engine's may depend on."""
import json

import numpy as np
import pytest

from matrix0_amd import analysis, reanalyse
from matrix0_amd import engine as eng
from matrix0_amd.data_writer import SelfplayShardWriter
from oracle import chess_py as ch
from tests import planes_cases as pc

CFG = {"seed": 5, "mcts": {"inference_batch_size": 8}, "selfplay": {"num_simulations": 32}}
MATE = "rnb1kbnr/pppp1ppp/8/4p3/6Pq/5P2/PPPPP2P/RNBQKBNR w KQkq - 1 3"
OVERFLOW_ID, TB_ID, NO_VISITS_ID = 1003, 1005, 1007


def _visits_for(i, k):
    return np.random.default_rng(int(i)).integers(0, 9, size=k).astype(np.int32) + (np.arange(k) == int(i) % k)


class _FakeEngine:
    """Stands in for eng.AnalysisEngine: submit_planes decodes on the host, queues the rows of status 0 and answers two per
    step, LAST queued first."""
    made = []

    def __init__(self, backend, cfg, **opts):
        self.cfg, self.queue, self.done, self.keeping, self.batches = cfg, [], [], False, []
        _FakeEngine.made.append(self)

    def keep_visits(self, on=True):
        self.keeping = bool(on)

    def submit_planes(self, planes, mask=None, sims=0, ids=None):
        d = pc.host_decode(planes, mask)
        self.batches.append(len(planes))
        for r in range(len(planes)):
            if d["status"][r] == 0:
                k = int(d["nlegal"][r])
                self.queue.append((int(ids[r]), k, d["idx"][r, :k].copy(), sims, ch.Board(d["fens"][r]).is_check()))
        return d["status"], d["flags"]

    def pending(self):
        return len(self.queue)

    def step(self, steps=1):
        for _ in range(2):
            if not self.queue:
                return
            i, k, idx, sims, check = self.queue.pop()
            r = {"id": i, "status": "ok", "nlegal": k, "overflow": False, "sims": sims, "root_n": sims, "evals": sims,
                 "value": 0.0, "root_q": ((i * 37) % 200 - 100) / 100.0, "lines": [], "policy_idx": np.zeros(0, np.int32),
                 "visits": np.zeros(0, np.int32)}
            if k == 0:
                r["status"] = "checkmate" if check else "stalemate"
            elif i == TB_ID:
                r.update(status="tablebase", root_q=-1.0, lines=[{"move": "x", "policy_index": int(idx[2]), "visits": 0}])
            else:
                r["overflow"] = i == OVERFLOW_ID
                if self.keeping:
                    r["policy_idx"] = idx
                    r["visits"] = np.zeros(k, np.int32) if i == NO_VISITS_ID else _visits_for(i, k)
            self.done.append(r)

    def poll(self, visits=False):
        assert visits
        return self.done.pop(0) if self.done else None

    def close(self):
        pass


@pytest.fixture
def analyzer(monkeypatch):
    _FakeEngine.made = []
    monkeypatch.setattr(eng, "AnalysisEngine", _FakeEngine)
    return analysis.Analyzer(None, CFG, slots=3)


def _rows():
    """A small shard: the en-passant positions, a mate, a saturated clock, three malformed rows; one-hot pi, z in {-1, 0, 1}."""
    fens = [f for f, _ in pc.EP_FENS] + [MATE, "4k3/8/8/8/8/8/4P3/4K3 w - - 120 90", ch.START_FEN, ch.START_FEN, ch.START_FEN]
    enc = [pc.encode(f) for f in fens]
    s, mask = np.stack([e[0] for e in enc]), np.stack([e[1] for e in enc])
    bad = {name: (p, m) for name, _, p, m in pc.malformed_rows()}
    n = len(fens)
    for row, name in ((n - 3, "piece_value_nan"), (n - 2, "mask_extra_bit")):
        s[row], mask[row] = bad[name]
    pi = np.zeros((n, 4672), np.float32)
    for r in range(n):
        on = np.flatnonzero(mask[r])
        pi[r, on[r % len(on)] if len(on) else 0] = 1.0
    z = np.array([(-1.0, 0.0, 1.0)[r % 3] for r in range(n)], np.float32)
    return fens, s, pi, z, mask


def test_target_rule_and_every_reason_to_keep(analyzer):
    fens, s, pi, z, mask = _rows()
    n = len(fens)
    ids = np.arange(1000, 1000 + n)
    before = (s.copy(), pi.copy(), z.copy(), mask.copy())
    pi2, z2, rep = reanalyse.reanalyse_arrays(s, pi, z, mask, sims=16, ids=ids, analyzer=analyzer)
    for a, b in zip(before, (s, pi, z, mask)):
        assert a.tobytes() == b.tobytes()                            # inputs untouched (one row holds a NaN)
    assert analyzer.engine.keeping
    mate, sat, nan_row, mm_row = len(pc.EP_FENS), len(pc.EP_FENS) + 1, n - 3, n - 2
    kept = {mate: "no_legal_move", sat: "halfmove_saturated", nan_row: "decode:piece_value", mm_row: "decode:mask_mismatch",
            OVERFLOW_ID - 1000: "arena_overflow", NO_VISITS_ID - 1000: "no_visits"}
    for row in range(n):
        i = int(ids[row])
        if row in kept:
            assert np.array_equal(pi2[row], pi[row]) and z2[row] == z[row], (row, kept[row])
            assert i in rep["kept_ids"][kept[row]], (row, kept[row])
        elif i == TB_ID:
            on = np.flatnonzero(mask[row])
            want = np.zeros(4672, np.float32); want[pc.host_decode(s[row][None], mask[row][None])["idx"][0, 2]] = 1.0
            assert np.array_equal(pi2[row], want) and z2[row] == -1.0 and on.size
        else:
            d = pc.host_decode(s[row][None], mask[row][None])
            k = int(d["nlegal"][0])
            v = _visits_for(i, k)
            want = np.zeros(4672, np.float32)
            want[d["idx"][0, :k]] = (v.astype(np.float64) / float(v.sum())).astype(np.float32)
            assert np.array_equal(pi2[row], want), row                # float32(n / total), nothing outside the children
            assert abs(float(pi2[row].sum(dtype=np.float64)) - 1.0) <= 1e-6
            assert not pi2[row][mask[row] == 0].any()
            assert z2[row] == z[row]                                  # value_mix = 0: z stays
    assert rep["rows"] == n and rep["kept"] == {v: 1 for v in kept.values()} and rep["mask_mismatches"] == 1
    assert rep["tablebase"] == 1 and rep["searched"] == n - len(kept) - 1
    assert rep["mean_kl"] > 0 and 0.0 <= rep["argmax_moved"] <= 1.0
    assert SelfplayShardWriter.validate_policy_targets(pi2)
    # the saturated row is searched on request
    pi3, _, rep3 = reanalyse.reanalyse_arrays(s, pi, z, mask, sims=16, ids=ids, analyzer=analyzer, search_saturated=True)
    assert "halfmove_saturated" not in rep3["kept"] and not np.array_equal(pi3[sat], pi[sat])
    others = [r for r in range(n) if r != sat]
    assert np.array_equal(pi3[others], pi2[others])
    # the batch size changes nothing
    pi4, z4, rep4 = reanalyse.reanalyse_arrays(s, pi, z, mask, sims=16, ids=ids, analyzer=analyzer, batch_rows=4)
    assert np.array_equal(pi4, pi2) and np.array_equal(z4, z2) and max(analyzer.engine.batches[-5:]) <= 4
    assert {k: v for k, v in rep4.items() if k != "kl_sum"} == {k: v for k, v in rep.items() if k != "kl_sum"}
    assert abs(rep4["kl_sum"] - rep["kl_sum"]) < 1e-9


def test_value_mix_blends_with_root_q_of_the_side_to_move(analyzer):
    fens, s, pi, z, mask = _rows()
    ids = np.arange(2000, 2000 + len(fens))
    for mix in (0.25, 1.0):
        _, z2, _ = reanalyse.reanalyse_arrays(s, pi, z, mask, sims=16, ids=ids, analyzer=analyzer, value_mix=mix)
        for row in range(len(pc.EP_FENS)):                              # rows that are searched
            q = ((int(ids[row]) * 37) % 200 - 100) / 100.0
            assert z2[row] == np.float32((1.0 - mix) * float(z[row]) + mix * q), (mix, row)
    assert reanalyse.blend_value(0.5, -1.0, 0.0) == np.float32(0.5)
    assert reanalyse.blend_value(1.0, -1.0, 0.5) == np.float32(0.0)    # same point of view: no sign flip
    with pytest.raises(ValueError):
        reanalyse.reanalyse_arrays(s, pi, z, mask, sims=16, analyzer=analyzer, value_mix=1.5)
    with pytest.raises(ValueError):
        reanalyse.reanalyse_arrays(s, pi, z, mask, sims=64, analyzer=analyzer)           # more than the arenas hold
    with pytest.raises(ValueError):
        reanalyse.reanalyse_arrays(s, pi, z, mask, sims=16, analyzer=analyzer, ids=np.zeros(len(fens), np.int64))
    assert reanalyse.policy_from_visits([], []) is None and reanalyse.policy_from_visits([3, 4], [0, 0]) is None
    idx, p = reanalyse.policy_from_visits([7, 9, 11], [1, 2, 0])
    assert idx.tolist() == [7, 9, 11] and p.dtype == np.float32 and p.tolist() == [np.float32(1 / 3), np.float32(2 / 3), 0.0]


def test_shards_ids_run_over_the_split_and_nothing_else_changes(analyzer, tmp_path):
    fens, s, pi, z, mask = _rows()
    n = len(fens)
    extra = np.arange(n, dtype=np.int32)

    def write(base, cuts):
        d = tmp_path / base
        d.mkdir()
        for k, (a, b) in enumerate(zip([0] + cuts, cuts + [n])):
            np.savez_compressed(d / f"shard_{k:03d}.npz", s=s[a:b], pi=pi[a:b], z=z[a:b].reshape(-1, 1), legal_mask=mask[a:b],
                                meta_row=extra[a:b])
        return d

    def read(out):
        rep = json.load(open(out / reanalyse.REPORT_NAME))
        shards = [np.load(sh["written"]) for sh in rep["shards"]]
        return rep, {k: np.concatenate([sh[k] for sh in shards]) for k in shards[0].files}

    one, three = write("one", []), write("three", [5, 11])
    rep1 = reanalyse.reanalyse_shards(one, tmp_path / "out1", analyzer=analyzer, sims=16, first_id=1000)
    rep3 = reanalyse.reanalyse_shards(three, tmp_path / "out3", analyzer=analyzer, sims=16, first_id=1000)
    (j1, d1), (j3, d3) = read(tmp_path / "out1"), read(tmp_path / "out3")
    assert len(j1["shards"]) == 1 and len(j3["shards"]) == 3 and [sh["first_id"] for sh in j3["shards"]] == [1000, 1005, 1011]
    for k in ("s", "pi", "z", "legal_mask", "meta_row"):
        assert d1[k].tobytes() == d3[k].tobytes() and d1[k].shape == d3[k].shape, k   # the split changes nothing
    assert d1["s"].tobytes() == s.tobytes() and d1["legal_mask"].tobytes() == mask.tobytes()
    assert d1["s"].dtype == np.float32 and d1["legal_mask"].dtype == np.uint8 and d1["z"].shape == (n, 1)
    assert np.array_equal(d1["meta_row"], extra)
    assert SelfplayShardWriter.validate_policy_targets(d1["pi"]) and not np.array_equal(d1["pi"], pi)
    for key in ("rows", "searched", "tablebase", "kept", "mask_mismatches", "argmax_moved_rows"):
        assert rep1[key] == rep3[key] == j1[key], key
    assert rep1["rows"] == n and rep1["kept"]["decode:mask_mismatch"] == 1 and rep1["sims"] == 16
    # the sources are as they were, and nothing is ever written in place
    with np.load(one / "shard_000.npz") as src:
        assert np.array_equal(src["pi"], pi)
    with pytest.raises(ValueError, match="in place"):
        reanalyse.reanalyse_shards(one, one, analyzer=analyzer, sims=16)


def test_command_line_arguments():
    ap = reanalyse.build_parser()
    a = ap.parse_args(["--config", "c.yaml", "--checkpoint", "k.pt", "--in", "a", "--out", "b"])
    assert (a.in_dir, a.out_dir, a.sims, a.value_mix, a.search_saturated, a.slots) == ("a", "b", None, 0.0, False, 256)
    a = ap.parse_args(["--config", "c", "--checkpoint", "k", "--in", "a", "--out", "b", "--sims", "200", "--value-mix", "0.5",
                       "--search-saturated"])
    assert (a.sims, a.value_mix, a.search_saturated) == (200, 0.5, True)
    with pytest.raises(SystemExit):
        ap.parse_args(["--config", "c.yaml", "--in", "a"])
