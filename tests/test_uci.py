"""The UCI front end (matrix0_amd/uci.py) without a GPU: the protocol against a stand-in engine in the style of
tests/test_analysis.py -- parsing of every command, option bounds, positions that are refused, the decision to reuse the held
tree, the time budget, the score conventions, the info / bestmove text, a stop before the first visit, and isready during a
search."""
import math

import pytest

from matrix0_amd import uci

START = uci.START_FEN


class _FakeEngine:
    """Stands in for a one-slot AnalysisEngine: a search gains `leaves` simulations per step (none in its first step, which
    expands the root), its best line gets every visit; the calls are logged."""

    def __init__(self, leaves=8, first_visit_after=1, terminal=None, tablebase=None):
        self.leaves, self.first_visit_after = leaves, first_visit_after
        self.terminal, self.tablebase = terminal, tablebase
        self.log, self.done, self.run, self.held_ids, self.closed = [], [], None, set(), False

    def _result(self):
        r = self.run
        visits = r["done"] if r["steps"] > self.first_visit_after else 0
        lines = [] if r["steps"] == 0 else [
            {"move": "e2e4", "policy_index": 1, "visits": visits, "prior": 0.5, "q": 0.5, "pv": ["e2e4", "e7e5", "g1f3"]},
            {"move": "d2d4", "policy_index": 2, "visits": 0, "prior": 0.3, "q": -0.5, "pv": ["d2d4"]}]
        return {"id": r["id"], "status": "ok", "nlegal": 20, "overflow": False, "sims": r["done"], "root_n": r["reused"] + r["done"],
                "evals": r["done"] + 1, "value": 0.1, "root_q": 0.2, "lines": lines}

    def _start(self, id, sims, keep, reused):
        if self.terminal:
            self.done.append({"id": id, "status": self.terminal, "nlegal": 0, "overflow": False, "sims": sims, "root_n": 0,
                              "evals": 0, "value": 0.0, "root_q": 0.0, "lines": []})
        elif self.tablebase:
            self.done.append(dict(self.tablebase, id=id))
        else:
            self.run = {"id": id, "sims": sims, "keep": keep, "done": 0, "steps": 0, "reused": reused}

    def submit(self, fen, ucis=(), sims=0, id=0, keep=False):
        self.log.append(("submit", fen, list(ucis), sims, id, keep))
        self._start(id, sims, keep, 0)

    def continue_search(self, held_id, ucis=(), sims=1, id=0, keep=False):
        self.log.append(("continue", held_id, list(ucis), sims, id, keep))
        assert held_id in self.held_ids
        self.held_ids.discard(held_id)
        reused = 0 if self.terminal or self.tablebase else 40
        self._start(id, sims, keep, reused)
        return reused

    def _finish(self):
        r, self.run = self.run, None
        if r["keep"]:
            self.held_ids.add(r["id"])

    def step(self, steps=1):
        self.log.append(("step",))
        r = self.run
        if r is None:
            return
        if r["steps"] > 0:
            r["done"] = min(r["sims"], r["done"] + self.leaves)
        r["steps"] += 1
        if r["done"] >= r["sims"]:
            self.done.append(self._result())
            self._finish()

    def peek(self, id):
        self.log.append(("peek", id))
        if self.run is None or self.run["id"] != id:
            raise ValueError("not running")
        return self._result()

    def stop(self, id):
        self.log.append(("stop", id))
        assert self.run is not None and self.run["id"] == id
        self.done.append(self._result())
        self._finish()

    def poll(self):
        return self.done.pop(0) if self.done else None

    def release(self, id):
        self.log.append(("release", id))
        self.held_ids.remove(id)

    def held(self):
        return len(self.held_ids)

    def pending(self):
        return 0 if self.run is None else 1

    def close(self):
        self.closed = True


class _Clock:
    def __init__(self):
        self.t = 0.0

    def __call__(self):
        return self.t


def _fen_after(fen, moves):
    """Host validation stand-in: a FEN needs six fields, moves are four or five characters; 'zzzz' is illegal.  The side to
    move flips with every move."""
    f = fen.split()
    if len(f) != 6 or f[1] not in "wb":
        raise ValueError("bad FEN")
    for m in moves:
        if len(m) not in (4, 5) or m == "zzzz":
            raise ValueError(f"Illegal move: {m}")
    if len(moves) % 2:
        f[1] = "b" if f[1] == "w" else "w"
    return " ".join(f)


def _uci(engine=None, cfg=None, **kw):
    out, clock = [], _Clock()
    e = engine or _FakeEngine()
    u = uci.UciEngine(e, cfg or {"selfplay": {"num_simulations": 256}, "mcts": {"inference_batch_size": 8}}, out=out.append,
                      clock=clock, step=lambda: (e.step(1), setattr(clock, "t", clock.t + 0.010)), fen_after=_fen_after, **kw)
    return u, e, out, clock


def _drive(u, limit=1000):
    """Pump until the search is over; the passes (engine steps) that took."""
    steps = lambda: [x[0] for x in u.engine.log].count("step")
    before, n = steps(), 0
    while u.pump():
        n += 1
        assert n < limit
    return steps() - before


def test_uci_and_isready():
    u, e, out, _ = _uci()
    u.command("uci")
    assert out[0] == "id name matrix0-amd" and out[1].startswith("id author ") and out[-1] == "uciok"
    opts = [ln for ln in out if ln.startswith("option name ")]
    assert "option name MultiPV type spin default 1 min 1 max 8" in opts
    assert "option name Leaves type spin default 8 min 1 max 96" in opts          # from mcts.inference_batch_size
    assert "option name MaxNodes type spin default 256 min 1 max 1000000" in opts  # from selfplay.num_simulations
    assert "option name Move Overhead type spin default 30 min 0 max 5000" in opts
    assert any(o.startswith("option name Tablebase type string") for o in opts)
    assert "option name TablebaseMen type spin default 4 min 3 max 4" in opts and len(opts) == 6
    del out[:]
    u.command("isready")
    u.command("   ")
    u.command("xyzzy 1 2")
    assert out == ["readyok", "info string unknown command: xyzzy"]


def test_setoption_and_its_bounds():
    u, e, out, _ = _uci()
    u.command("setoption name MultiPV value 3")
    u.command("setoption name move overhead value 100")
    u.command("setoption name Leaves value 96")
    u.command("setoption name Tablebase value /some/where/tb 3.bin")
    u.command("setoption name TablebaseMen value 3")
    assert out == [] and u.options == {"MultiPV": 3, "Move Overhead": 100, "MaxNodes": 256, "Leaves": 96,
                                       "Tablebase": "/some/where/tb 3.bin", "TablebaseMen": 3}
    assert u.dirty
    for line, word in (("setoption name MultiPV value 0", "[1, 8]"), ("setoption name MultiPV value 9", "[1, 8]"),
                       ("setoption name Leaves value 97", "[1, 96]"), ("setoption name Leaves value 0", "[1, 96]"),
                       ("setoption name MaxNodes value 0", "[1, 1000000]"), ("setoption name TablebaseMen value 5", "[3, 4]"),
                       ("setoption name Move Overhead value -1", "[0, 5000]"), ("setoption name MultiPV value many", "integer"),
                       ("setoption name Hash value 16", "unknown option"), ("setoption value 3", "needs a name")):
        del out[:]
        u.command(line)
        assert len(out) == 1 and out[0].startswith("info string") and word in out[0], line
    assert u.options["MultiPV"] == 3 and u.options["Leaves"] == 96 and u.options["TablebaseMen"] == 3


def test_changed_engine_options_rebuild_the_engine_before_the_next_search():
    made = []

    def rebuild(options):
        made.append(options)
        e2 = _FakeEngine()
        return e2, lambda: e2.step(1)

    u, e, out, _ = _uci(rebuild=rebuild)
    u.command("go nodes 8")
    _drive(u)
    assert made == [] and u.held is not None
    u.command("setoption name MaxNodes value 64")
    u.command("go nodes 100")
    assert e.closed and len(made) == 1 and made[0]["MaxNodes"] == 64 and u.engine is not e
    assert u.engine.log[0] == ("submit", START, [], 64, 2, True)                   # clipped to MaxNodes; the old tree is gone
    _drive(u)
    u.command("go nodes 8")
    assert len(made) == 1


def test_position_parsing_and_refusals():
    u, e, out, _ = _uci()
    u.command("position startpos moves e2e4 e7e5")
    assert (u.base, u.moves) == (START, ["e2e4", "e7e5"]) and out == []
    fen = "8/8/8/4k3/8/8/1r6/K1Q5 w - - 0 1"
    u.command(f"position fen {fen}")
    assert (u.base, u.moves) == (fen, [])
    u.command(f"position fen {fen} moves c1b2")
    assert (u.base, u.moves) == (fen, ["c1b2"])
    for line in ("position fen 8/8/8 w", "position startpos moves e2e4 zzzz", "position", "position startpos e2e4",
                 f"position fen {fen} moves c1b2 toolong"):
        del out[:]
        u.command(line)
        assert len(out) == 1 and out[0].startswith("info string position"), line
        assert (u.base, u.moves) == (fen, ["c1b2"]), line


def test_go_arguments():
    args, bad = uci.parse_go("wtime 1000 btime 2000 winc 10 binc 20 movestogo 5".split())
    assert args == {"wtime": 1000, "btime": 2000, "winc": 10, "binc": 20, "movestogo": 5} and bad == []
    assert uci.parse_go(["infinite"]) == ({"infinite": True}, [])
    assert uci.parse_go("nodes 128".split()) == ({"nodes": 128}, [])
    assert uci.parse_go("movetime 250".split()) == ({"movetime": 250}, [])
    args, bad = uci.parse_go("searchmoves e2e4 d2d4 nodes 5 ponder depth 3 mate 2".split())
    assert args == {"searchmoves": ["e2e4", "d2d4"], "nodes": 5, "ponder": True, "depth": 3, "mate": 2} and bad == []
    assert uci.parse_go("nodes x frob".split()) == ({}, ["nodes", "x", "frob"])
    u, e, out, _ = _uci()
    u.command("go depth 3 mate 2 ponder searchmoves e2e4 nodes 16")
    assert [o for o in out if "ignored" in o] == [f"info string go {w} is not supported and ignored"
                                                  for w in ("depth", "mate", "searchmoves", "ponder")]
    assert e.log[0] == ("submit", START, [], 16, 1, True)


def test_the_reuse_decision():
    held = {"id": 1, "base": START, "moves": ["e2e4", "e7e5"]}
    moves9 = ["e2e4", "e7e5"] + ["g1f3", "g8f6", "f3g1", "f6g8"] * 2 + ["g1f3"]
    assert uci.reuse_moves(held, START, ["e2e4", "e7e5"]) == []
    assert uci.reuse_moves(held, START, ["e2e4", "e7e5", "g1f3", "b8c6"]) == ["g1f3", "b8c6"]
    assert uci.reuse_moves(held, START, moves9[:10]) == moves9[2:10] and len(moves9[2:10]) == 8
    assert uci.reuse_moves(held, START, moves9) is None                            # nine moves further
    assert uci.reuse_moves(held, START, ["e2e4"]) is None                          # shorter
    assert uci.reuse_moves(held, START, ["d2d4", "e7e5", "g1f3"]) is None          # another line
    assert uci.reuse_moves(held, "8/8/8/4k3/8/8/1r6/K1Q5 w - - 0 1", ["e2e4", "e7e5"]) is None
    assert uci.reuse_moves(None, START, []) is None
    # through the protocol
    u, e, out, _ = _uci()
    u.command("position startpos moves e2e4 e7e5")
    u.command("go nodes 16")
    _drive(u)
    assert u.held == {"id": 1, "base": START, "moves": ["e2e4", "e7e5"]} and e.held_ids == {1}
    u.command("position startpos moves e2e4 e7e5 g1f3 b8c6")
    u.command("go nodes 16")
    assert e.log[-1] == ("continue", 1, ["g1f3", "b8c6"], 16, 2, True)
    assert "info string tree reused: 40 nodes kept over 2 moves" in out
    _drive(u)
    u.command("go nodes 16")                                                       # the same position again: 0 moves
    assert e.log[-1] == ("continue", 2, [], 16, 3, True)
    _drive(u)
    u.command("position startpos moves " + " ".join(moves9 + ["g8f6", "f3g1", "f6g8"] * 1 + ["b1c3"] * 0))
    u.command("go nodes 16")                                                       # 2 + 9 + ... moves behind the held 4
    assert e.log[-2:] == [("release", 3), ("submit", START, moves9 + ["g8f6", "f3g1", "f6g8"], 16, 4, True)]
    _drive(u)
    u.command("position fen 8/8/8/4k3/8/8/1r6/K1Q5 w - - 0 1")
    u.command("go nodes 16")                                                       # another base
    assert e.log[-2][0] == "release" and e.log[-1][0] == "submit"
    _drive(u)
    assert e.held_ids == {5}
    u.command("ucinewgame")
    assert e.log[-1] == ("release", 5) and u.held is None and e.held_ids == set()
    u.command("go nodes 16")
    assert e.log[-1][0] == "submit"


def test_time_budget():
    tb = uci.time_budget_ms
    cases = [    # remaining, inc, movestogo, overhead -> budget
        ((60000, 0, None, 0), 2000.0),            # 1/30 of the clock
        ((60000, 1000, None, 30), 2720.0),        # + 3/4 of the increment - overhead
        ((60000, 0, 1, 0), 30000.0),              # one move to go: never more than half of what is left
        ((60000, 0, 10, 50), 5950.0),
        ((60000, 0, 0, 0), 2000.0),               # movestogo 0 counts as not given
        ((1000, 10000, None, 0), 500.0),          # a large increment: still half of the remaining time
        ((100, 0, None, 500), 0.0),               # overhead larger than the budget
        ((0, 0, None, 0), 0.0),
    ]
    for args, want in cases:
        assert tb(*args) == pytest.approx(want), args
    assert tb(0, 0, None, 30, movetime=1000) == 970.0
    assert tb(60000, 0, None, 300, movetime=100) == 0.0
    assert tb(60000, 0, None, 0) == tb(60000, 0, None, 0)


def test_score_conventions(monkeypatch):
    assert uci.cp_from_q(0.0) == 0
    assert uci.cp_from_q(0.5) == round(90 * math.tan(1.5637541897 * 0.5)) == 89
    assert uci.cp_from_q(-0.5) == -89
    assert uci.cp_from_q(1.0) == round(90 * math.tan(1.5637541897)) == 12780 and uci.cp_from_q(-1.0) == -12780
    assert uci.cp_from_q(7.0) == 12780 and uci.cp_from_q(-7.0) == -12780            # q is held to [-1, 1] first
    assert (uci.CP_SCALE, uci.CP_ANGLE, uci.CP_CLIP) == (90.0, 1.5637541897, 12800)
    monkeypatch.setattr(uci, "CP_ANGLE", 1.5707)                                    # a steeper mapping runs into the clip
    assert uci.cp_from_q(1.0) == 12800 and uci.cp_from_q(-1.0) == -12800 and uci.cp_from_q(0.0) == 0
    # distance to mate in plies -> moves, negative for the side that is mated
    assert [uci.mate_score(d, False) for d in (1, 3, 5, 21)] == [1, 2, 3, 11]
    assert [uci.mate_score(d, True) for d in (2, 4, 6, 0)] == [-1, -2, -3, 0]


def test_info_and_bestmove_text():
    u, e, out, clock = _uci()
    u.command("setoption name MultiPV value 2")
    u.command("go nodes 16")
    assert out == []
    n = _drive(u)
    assert n == 3                                                # the root's expansion, then two passes of 8
    assert out == ["info depth 3 multipv 1 score cp 89 nodes 16 nps 533 time 30 pv e2e4 e7e5 g1f3",
                   "info depth 1 multipv 2 score cp -89 nodes 16 nps 533 time 30 pv d2d4",
                   "bestmove e2e4 ponder e7e5"]
    assert not u.searching() and u.pump() is False
    # a long search prints its lines every 500 ms and once at the end
    del out[:]
    u.command("setoption name MultiPV value 1")
    u.command("go nodes 256")
    _drive(u)                                                    # 10 ms a pass, 33 passes
    infos = [o for o in out if o.startswith("info depth")]
    assert len(infos) == 1 and out[-1].startswith("bestmove e2e4")
    del out[:]
    u.step = lambda: (e.step(1), setattr(clock, "t", clock.t + 0.2))
    u.command("go nodes 256")
    _drive(u)                                                    # 200 ms a pass: a line after every third pass, the last with the answer
    infos = [o for o in out if o.startswith("info depth")]
    assert len(infos) == 10 + 1 and " nodes 296 " in infos[-1] and out[-1].startswith("bestmove")
    times = [int(o.split(" time ")[1].split()[0]) for o in infos]
    assert all(b - a >= 500 for a, b in zip(times[:-2], times[1:-1]))


def test_no_legal_moves_and_tablebase_scores():
    for status in ("checkmate", "stalemate"):
        u, e, out, _ = _uci(_FakeEngine(terminal=status))
        u.command("go nodes 16")
        assert out == ["bestmove 0000"] and not u.searching() and u.held is None
    tb = {"status": "tablebase", "nlegal": 3, "overflow": False, "sims": 0, "root_n": 0, "evals": 0, "value": 0.0, "root_q": 1.0,
          "dtm": 3, "lines": [
              {"move": "a1a2", "policy_index": 1, "visits": 0, "prior": 0.0, "q": 1.0, "pv": ["a1a2", "h8g8", "a2a8"], "dtm": 2},
              {"move": "a1b1", "policy_index": 2, "visits": 0, "prior": 0.0, "q": 0.0, "pv": ["a1b1"], "dtm": 0},
              {"move": "a1c1", "policy_index": 3, "visits": 0, "prior": 0.0, "q": -1.0, "pv": ["a1c1", "h8g8"], "dtm": 3}]}
    u, e, out, _ = _uci(_FakeEngine(tablebase=tb))
    u.command("setoption name MultiPV value 8")
    u.command("go infinite")
    assert [o.split(" nodes ")[0] for o in out[:3]] == ["info depth 3 multipv 1 score mate 2", "info depth 1 multipv 2 score cp 0",
                                                        "info depth 2 multipv 3 score mate -2"]
    assert out[3] == "bestmove a1a2 ponder h8g8" and u.held is None and len(out) == 4


def test_stop_before_the_first_visit_keeps_stepping():
    e = _FakeEngine(first_visit_after=3)                         # the best line has no visit until the fifth pass
    u, e, out, _ = _uci(e)
    u.command("go infinite")
    assert u.pump() and out == []
    u.command("stop")
    n = _drive(u)
    assert n == 3 and [x[0] for x in e.log].count("stop") == 1   # three more passes: four in all
    assert e.log[-1] == ("stop", 1) and e.log[-2] == ("peek", 1) and out[-1] == "bestmove e2e4 ponder e7e5"
    visits = [ln for ln in out if ln.startswith("info depth")]
    assert len(visits) == 1 and " nodes 24 " in visits[0]
    # with a visit on the board the stop is immediate: no further pass
    u.command("go infinite")
    for _ in range(5):
        u.pump()
    steps = [x[0] for x in e.log].count("step")
    u.command("stop")
    assert u.pump() is False and [x[0] for x in e.log].count("step") == steps and out[-1].startswith("bestmove")


def test_go_infinite_runs_to_max_nodes_and_time_limits_stop_earlier():
    u, e, out, clock = _uci()
    u.command("go infinite")
    assert _drive(u) == 33 and e.log[0] == ("submit", START, [], 256, 1, True)
    # movetime 105 with 30 ms overhead and 10 ms passes: a pass starts only while elapsed + longest pass <= 75 ms (at 0 .. 60)
    u.command("ucinewgame")
    del out[:], e.log[:]
    clock.t = 0.0
    u.command("go movetime 105")
    _drive(u)
    assert [x[0] for x in e.log].count("step") == 7 and e.log[-1] == ("stop", 2)
    assert out[-1].startswith("bestmove") and " time 70 " in out[-2]
    # the clock of the side to move: Black after one move
    u.command("ucinewgame")
    del e.log[:]
    clock.t = 0.0
    u.command("position startpos moves e2e4")
    u.command("go wtime 100000 btime 3150 winc 0 binc 0")        # 3150 / 30 - 30 = 75 ms
    _drive(u)
    assert [x[0] for x in e.log].count("step") == 7


def test_isready_is_answered_during_a_search_and_other_commands_wait():
    u, e, out, _ = _uci()
    u.command("go infinite")
    u.pump()
    u.command("isready")
    assert out == ["readyok"]
    del out[:]
    u.command("position startpos moves e2e4")
    u.command("go nodes 4")
    u.command("ucinewgame")
    u.command("setoption name Leaves value 4")
    assert [o.split(" ignored")[0] for o in out[:3]] == ["info string position", "info string go", "info string ucinewgame"]
    assert "cannot change during a search" in out[3] and u.moves == [] and u.options["Leaves"] == 8
    u.command("quit")
    assert u.quit and not u.searching() and e.log[-1] == ("stop", 1) and not any(o.startswith("bestmove") for o in out)


def test_command_line_arguments():
    ap = uci.build_parser()
    a = ap.parse_args(["--config", "c.yaml", "--checkpoint", "k.pt"])
    assert (a.config, a.checkpoint, a.device) == ("c.yaml", "k.pt", 0)
    assert ap.parse_args(["--config", "c", "--checkpoint", "k", "--device", "3"]).device == 3
    with pytest.raises(SystemExit):
        ap.parse_args(["--config", "c.yaml"])


def test_command_line_loop_reads_stdin_and_searches_on_the_main_thread(tmp_path, monkeypatch, capsys):
    import io
    import json
    import sys
    import threading
    import matrix0_amd.backend as backend
    from matrix0_amd import engine as eng
    seen = {"threads": set(), "closed": []}

    class _Backend:
        @classmethod
        def from_checkpoint(cls, model_cfg, path, device):
            seen["args"] = (model_cfg, path, device)
            return cls()

        def close(self):
            seen["closed"].append("backend")

    class _Engine(_FakeEngine):
        def step(self, steps=1):
            seen["threads"].add(threading.current_thread() is threading.main_thread())
            super().step(steps)

        def close(self):
            seen["closed"].append("engine")

    def make(be, cfg, options):
        seen["options"] = dict(options)
        e = _Engine()
        return e, (lambda: e.step(1))

    monkeypatch.setattr(backend, "M0Backend", _Backend)
    monkeypatch.setattr(uci, "make_engine", make)
    monkeypatch.setattr(eng, "fen_after", _fen_after)
    cfgp = tmp_path / "c.json"
    cfgp.write_text(json.dumps({"model": {"channels": 320}, "selfplay": {"num_simulations": 64}, "mcts": {"inference_batch_size": 8}}))
    monkeypatch.setattr(sys, "stdin", io.StringIO("uci\nisready\nposition startpos moves e2e4\ngo nodes 32\n"))
    assert uci.main(["--config", str(cfgp), "--checkpoint", "k.pt", "--device", "2"]) == 0     # end of input: the search is finished first
    out = capsys.readouterr().out.strip().split("\n")
    assert seen["args"] == ({"channels": 320}, "k.pt", 2) and seen["options"]["MaxNodes"] == 64 and seen["options"]["Leaves"] == 8
    assert "uciok" in out and "readyok" in out and out[-1] == "bestmove e2e4 ponder e7e5" and " nodes 32 " in out[-2]
    assert seen["threads"] == {True} and seen["closed"] == ["engine", "backend"]
    # quit ends the loop at once, without a bestmove
    monkeypatch.setattr(sys, "stdin", io.StringIO("go infinite\nquit\n"))
    assert uci.main(["--config", str(cfgp), "--checkpoint", "k.pt"]) == 0
    assert "bestmove" not in capsys.readouterr().out
