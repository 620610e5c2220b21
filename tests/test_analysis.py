"""Host side of the batched position analysis (no GPU): Analyzer's bookkeeping
(submission order restored from completion order, ids, argument checks) against a stand-in engine, suite_accuracy, and the
command line's arguments and output lines."""
import json

import pytest

from matrix0_amd import analysis
from matrix0_amd import engine as eng


def test_game_structs_are_untouched():
    assert [n for n, _ in eng.SelfplayCfg._fields_][-3:] == ["tail_split", "arena_eval_cache", "arena_paired_openings"]
    assert [n for n, _ in eng.GameRecord._fields_][-2:] == ["owner", "start_fen"]


class _FakeAnalysisEngine:
    """Stands in for eng.AnalysisEngine: answers every submission with a line that names its id, two per step, LAST submitted
    first -- completion order is the reverse of submission order."""
    made = []

    def __init__(self, backend, cfg, **opts):
        self.cfg, self.opts, self.queue, self.done, self.submitted, self.closed = cfg, opts, [], [], [], False
        _FakeAnalysisEngine.made.append(self)

    def submit(self, fen, ucis=(), sims=0, id=0):
        self.queue.append((fen, list(ucis), sims, id))
        self.submitted.append((fen, list(ucis), sims, id))

    def pending(self):
        return len(self.queue)

    def step(self, steps=1):
        for _ in range(2):
            if self.queue:
                fen, ucis, sims, i = self.queue.pop()
                lines = [{"move": f"m{i}_{k}", "policy_index": k, "visits": 9 - k, "prior": 0.1, "q": 0.0, "pv": [f"m{i}_{k}"]}
                         for k in range(self.opts["multipv"])]
                self.done.append({"id": i, "status": "ok", "nlegal": 20, "overflow": False, "sims": sims, "root_n": sims,
                                  "evals": 1, "value": 0.0, "root_q": 0.0, "lines": lines})

    def poll(self):
        return self.done.pop(0) if self.done else None

    def stats(self):
        return {"evals": 0}

    def close(self):
        self.closed = True


@pytest.fixture
def fake_engine(monkeypatch):
    _FakeAnalysisEngine.made = []
    monkeypatch.setattr(eng, "AnalysisEngine", _FakeAnalysisEngine)
    return _FakeAnalysisEngine.made


CFG = {"seed": 5, "mcts": {"inference_batch_size": 8}, "selfplay": {"num_simulations": 32}}


def test_analyse_restores_submission_order(fake_engine):
    an = analysis.Analyzer(None, CFG, slots=3, multipv=2, pv_len=4)
    e = fake_engine[-1]
    assert (e.cfg.concurrent_games, e.cfg.inference_batch_size, e.cfg.num_simulations, e.cfg.record_games) == (3, 8, 32, 0)
    assert e.opts == {"multipv": 2, "pv_len": 4, "dirichlet": False}
    positions = ["fenA", ("fenB", ["e2e4", "e7e5"]), "fenC", "fenD", ("fenE", [])]
    out = an.analyse(positions, sims=16)
    assert [r["id"] for r in out] == [0, 1, 2, 3, 4]
    assert [r["fen"] for r in out] == ["fenA", "fenB", "fenC", "fenD", "fenE"]
    assert out[1]["moves"] == ["e2e4", "e7e5"] and out[0]["moves"] == []
    assert [r["lines"][0]["move"] for r in out] == [f"m{i}_0" for i in range(5)]
    assert e.submitted[1] == ("fenB", ["e2e4", "e7e5"], 16, 1)
    # caller's ids, any order
    out = an.analyse(["x", "y", "z"], sims=8, ids=[30, 10, 20])
    assert [r["id"] for r in out] == [30, 10, 20] and [r["fen"] for r in out] == ["x", "y", "z"]
    # policy mode submits sims = 0 and cuts the lines to topk
    out = an.evaluate(["p", "q"], topk=1)
    assert [s[2] for s in e.submitted[-2:]] == [0, 0] and all(len(r["lines"]) == 1 for r in out)
    assert len(an.evaluate(["p"])[0]["lines"]) == 2
    with pytest.raises(ValueError):
        an.evaluate(["p"], topk=3)                       # more than multipv
    with pytest.raises(ValueError):
        an.analyse(["p"], sims=64)                       # more than the arenas were sized for
    with pytest.raises(ValueError):
        an.analyse(["p", "q"], sims=8, ids=[1, 1])
    with pytest.raises(ValueError):
        analysis.Analyzer(None, CFG, multipv=9)
    an.close()
    assert e.closed
    an = analysis.Analyzer(None, CFG, slots=2, max_sims=500)
    assert fake_engine[-1].cfg.num_simulations == 500


def _res(*moves):
    return {"lines": [{"move": m} for m in moves]}


def test_suite_accuracy():
    results = [_res("e2e4", "d2d4", "g1f3"), _res("a7a6", "e7e5"), _res(), _res("h2h4", "a2a4", "b2b4", "c2c4")]
    best = ["e2e4", "e7e5", "a1a2", "c2c4"]
    acc = analysis.suite_accuracy(results, best)
    assert acc == {"n": 4, "top1": 0.25, "top3": 0.5}
    assert analysis.suite_accuracy(results, best, k=(2, 4)) == {"n": 4, "top2": 0.5, "top4": 0.75}
    assert analysis.suite_accuracy([], []) == {"n": 0, "top1": 0.0, "top3": 0.0}
    with pytest.raises(ValueError):
        analysis.suite_accuracy(results, best[:2])


def test_command_line_arguments_and_output(tmp_path, fake_engine, monkeypatch, capsys):
    ap = analysis.build_parser()
    a = ap.parse_args(["--config", "c.yaml", "--checkpoint", "k.pt", "--fens", "f.txt"])
    assert (a.sims, a.multipv, a.pv_len, a.slots, a.device) == (None, 1, 8, 256, 0)
    a = ap.parse_args(["--config", "c", "--checkpoint", "k", "--fens", "f", "--sims", "200", "--multipv", "3"])
    assert (a.sims, a.multipv) == (200, 3)
    with pytest.raises(SystemExit):
        ap.parse_args(["--config", "c.yaml"])
    fens = tmp_path / "f.txt"
    fens.write_text("# comment\nfenA w - - 0 1\n\nfenB w - - 0 1 moves e2e4 e7e5   # trailing\n")
    assert analysis.read_positions(str(fens)) == ["fenA w - - 0 1", ("fenB w - - 0 1", ["e2e4", "e7e5"])]
    cfgp = tmp_path / "c.yaml"
    cfgp.write_text("seed: 3\nmodel: {channels: 320}\nmcts: {inference_batch_size: 8}\nselfplay: {num_simulations: 32}\n")
    assert analysis.load_config(str(cfgp))["model"] == {"channels": 320}
    seen = {}

    class _Backend:
        @classmethod
        def from_checkpoint(cls, model_cfg, path, device):
            seen["args"] = (model_cfg, path, device)
            return cls()

    import matrix0_amd.backend as backend
    monkeypatch.setattr(backend, "M0Backend", _Backend)
    assert analysis.main(["--config", str(cfgp), "--checkpoint", "k.pt", "--fens", str(fens), "--sims", "16", "--multipv", "2"]) == 0
    assert seen["args"] == ({"channels": 320}, "k.pt", 0)
    lines = capsys.readouterr().out.strip().split("\n")
    assert len(lines) == 2
    rows = [json.loads(x) for x in lines]
    assert list(rows[0]) == ["fen", "moves", "status", "nlegal", "sims", "root_n", "root_q", "value", "evals", "lines"]
    assert rows[1]["fen"] == "fenB w - - 0 1" and rows[1]["moves"] == ["e2e4", "e7e5"] and rows[1]["sims"] == 16
    assert [ln["move"] for ln in rows[1]["lines"]] == ["m1_0", "m1_1"] and rows[0]["lines"][0]["pv"] == ["m0_0"]
    assert fake_engine[-1].cfg.num_simulations == 16 and fake_engine[-1].closed
    # --sims 0: policy mode
    assert analysis.main(["--config", str(cfgp), "--checkpoint", "k.pt", "--fens", str(fens), "--sims", "0"]) == 0
    assert [s[2] for s in fake_engine[-1].submitted] == [0, 0]
