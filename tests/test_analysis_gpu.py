"""The analysis engine on the GPU (m0_analysis_*: csrc/capi_analysis.hip, csrc/analysis_kernels.hip) against the oracle
restatement of the reference's MCTS.run (oracle/mcts_ref.py), with the random streams and the evaluator of
tests/test_search_gpu.py: the lines (root children by visits, ties by move order -- the first-maximum rule of arena.py:73-106)
and the principal variations are derived here from the oracle's own tree; moves, policy indices, visit counts, root_n and PVs
must be identical, priors and q within 1e-6 (the tolerance of test_search_gpu._compare).  Then: move history reaches the
search, a result does not depend on the slot, the fused step equals the split step bit for bit on the 320-wide network
(bitwise batch invariant, tests/test_timed_path_gpu.py), and the policy mode against the host's softmax."""
import functools
import gzip
import json
import os

import numpy as np
import pytest

from oracle import chess_py as ch
from oracle import mcts_ref as ref
from oracle import net_ref
from tests.fake_net import FakeNet
from tests.test_search_gpu import FENS, MCTS
from tests.test_timed_path_gpu import NET

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIMS, LEAVES, MULTIPV, PV_LEN = 64, 8, 8, 16
MANY_MOVES = "R6R/3Q4/1Q4Q1/4Q3/2Q4Q/Q4Q2/pp1Q4/kBNN1KB1 w - - 0 1"     # 218 legal moves: 4 children on a lane
ONE_MOVE = "8/8/8/8/8/5k2/7q/7K w - - 0 1"                              # multipv > number of children
STALEMATE = "7k/5Q2/5K2/8/8/8/8/8 b - - 0 1"
CHECKMATE = "rnb1kbnr/pppp1ppp/8/4p3/6Pq/5P2/PPPPP2P/RNBQKBNR w KQkq - 1 3"
SHUFFLE = ["g1f3", "g8f6", "f3g1", "f6g8"]


@functools.lru_cache(maxsize=None)
def _fixture_rows():
    return json.load(gzip.open(os.path.join(GOLDEN, "stockfish_best_moves.json.gz"), "rt"))


def _positions():
    return list(FENS) + [MANY_MOVES, ONE_MOVE, STALEMATE, CHECKMATE] + [fen for fen, _ in _fixture_rows()[:20]]


def _cfg(sims=SIMS, leaves=LEAVES):
    return {"seed": 1234, "mcts": dict(MCTS, inference_batch_size=leaves), "selfplay": {"num_simulations": sims}}


def _oracle_lines(root, multipv, pv_len):
    """Expected lines of a searched root: children by (more visits, earlier in move order); behind each the most visited
    child, first maximum, until an unexpanded node, a node without visited children, or pv_len moves."""
    kids = list(root.children.values())
    lines = []
    for i in sorted(range(len(kids)), key=lambda i: (-kids[i].n, i))[:multipv]:
        node = kids[i]
        pv = [node.move.uci()]
        while len(pv) < pv_len and node.expanded and node.children:
            best = None
            for c in node.children.values():
                if best is None or c.n > best.n:
                    best = c
            if best.n == 0:
                break
            pv.append(best.move.uci())
            node = best
        lines.append({"move": kids[i].move.uci(), "policy_index": kids[i].move_idx, "visits": kids[i].n,
                      "prior": kids[i].prior, "q": kids[i].q, "pv": pv})
    return lines


def _oracle_run(fen, ucis, uid, dirichlet, sharp, sims=SIMS, leaves=LEAVES):
    m = dict(MCTS, inference_batch_size=leaves)
    cfg = ref.MCTSConfig.from_dict(dict(m, use_tt=False, virtual_loss_active=True, dirichlet_plies=(30 if dirichlet else 0),
                                        numerics="engine"))
    o = ref.MCTS(cfg, FakeNet(seed=3, sharp=sharp).infer_np, seed=1234, game=uid)
    b = ch.Board(fen)
    for u in ucis:
        b.push(ch.Move.from_uci(u))
    if not b.legal_moves:
        return {"status": "checkmate" if b.is_checkmate() else "stalemate", "lines": [], "evals": 0, "root_n": 0, "nlegal": 0}
    if b.is_game_over():
        # drawn by rule with legal moves left (three rows of the fixture are bare-minor-piece endings): run() answers without
        # a tree, the engine answers only mate and stalemate itself and searches these -- the steps of run() behind its test
        root = ref.Node()
        logits, v = o._infer_one(b)
        o.expand(root, b, logits, is_root=True)
        if dirichlet:
            o.add_dirichlet(root)
        o.run_batched(b, root, sims)
        rq = float(root.q) if root.n > 0 else float(v)
    else:
        _, _, rq = o.run(b, num_simulations=sims, ply=0)
        root = o._last_root
    return {"status": "ok", "lines": _oracle_lines(root, MULTIPV, PV_LEN), "evals": o.evals, "root_n": root.n, "root_q": rq,
            "nlegal": len(b.legal_moves), "counts": [c.n for c in root.children.values()]}


@functools.lru_cache(maxsize=None)
def _oracle_set(dirichlet):
    """The shared expectation of the position set (computed once per Dirichlet setting, never modified)."""
    return tuple(_oracle_run(fen, [], i, dirichlet, 8.0) for i, fen in enumerate(_positions()))


def _check(got, want, tag):
    assert got["status"] == want["status"], tag
    assert got["nlegal"] == want["nlegal"] and got["root_n"] == want["root_n"] and got["evals"] == want["evals"], tag
    assert [ln["move"] for ln in got["lines"]] == [ln["move"] for ln in want["lines"]], tag
    assert [ln["policy_index"] for ln in got["lines"]] == [ln["policy_index"] for ln in want["lines"]], tag
    assert [ln["visits"] for ln in got["lines"]] == [ln["visits"] for ln in want["lines"]], tag
    assert [ln["pv"] for ln in got["lines"]] == [ln["pv"] for ln in want["lines"]], tag
    if want["lines"]:
        np.testing.assert_allclose([ln["prior"] for ln in got["lines"]], [ln["prior"] for ln in want["lines"]], rtol=0, atol=1e-6)
        np.testing.assert_allclose([ln["q"] for ln in got["lines"]], [ln["q"] for ln in want["lines"]], rtol=0, atol=1e-6)
        assert abs(got["root_q"] - want["root_q"]) < 1e-6, tag
        assert not got["overflow"] and got["sims"] == SIMS, tag


def _ext(slots, dirichlet=False, sharp=8.0, **kw):
    from matrix0_amd import analysis
    return analysis.AnalyzerExt(FakeNet(seed=3, sharp=sharp).infer_np, _cfg(), slots=slots, multipv=MULTIPV, pv_len=PV_LEN,
                                dirichlet=dirichlet, **kw)


@pytest.mark.parametrize("dirichlet", [True, False])
def test_lines_and_pvs_match_the_oracle(dirichlet):
    positions = _positions()
    assert len(positions) == 30
    an = _ext(3, dirichlet)                               # 3 slots for 30 positions: every slot is refilled many times
    got = an.analyse(positions, SIMS)
    st = an.stats()
    an.close()
    want = _oracle_set(dirichlet)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g["id"] == i and g["fen"] == positions[i]
        _check(g, w, (i, positions[i]))
    # the shapes the set is there for
    many, one = got[len(FENS)], got[len(FENS) + 1]
    assert many["nlegal"] == 218 and len(many["lines"]) == MULTIPV and one["nlegal"] == 1 and len(one["lines"]) == 1
    assert any(len(ln["pv"]) > 2 for g in got for ln in g["lines"]) and any(len(ln["pv"]) == 1 for g in got for ln in g["lines"])
    # terminal roots: answered on the host, no evaluation, no slot
    stale, mate = got[len(FENS) + 2], got[len(FENS) + 3]
    assert (stale["status"], stale["lines"], stale["evals"]) == ("stalemate", [], 0)
    assert (mate["status"], mate["lines"], mate["evals"]) == ("checkmate", [], 0)
    assert st["evals"] == sum(w["evals"] for w in want)


def test_move_history_reaches_the_search():
    """A position submitted with the moves that led to it is searched with their repetition window.

    The case the feature's specification names -- the start position after g1f3 g8f6 f3g1 f6g8 g1f3 g8f6 f3g1 against the
    same position as a bare FEN -- is kept: the engine must equal the oracle board with the pushed moves.  The specification
    also expects the two results to differ, which the reference's own rules rule out: the search ends a line on a FIVEfold
    repetition (board.is_game_over(), mcts.py:747), after seven moves no position has occurred more than twice, and the
    oracle returns the same 64-simulation tree with and without the moves (asserted below).  The difference is therefore
    asserted where the rules produce one: after fifteen moves of the same shuffle the position has occurred four times, every
    return to it inside the search is a terminal draw, and oracle and engine both change their counts."""
    from matrix0_amd import engine as eng
    start = ch.START_FEN
    short, long = SHUFFLE + SHUFFLE[:3], SHUFFLE * 3 + SHUFFLE[:3]
    fen_short, fen_long = eng.fen_after(start, short), eng.fen_after(start, long)
    # a flat policy (sharp 0.5) spreads 64 simulations over the moves, the knight's way back among them; the pair of a
    # position shares its id, hence its random streams: the history is the only difference
    an = _ext(2, sharp=0.5)
    with_short, with_long = an.analyse([(start, short), (start, long)], SIMS, ids=[77, 80])
    bare_short, bare_long = an.analyse([fen_short, fen_long], SIMS, ids=[77, 80])
    an.close()
    o_with_short, o_bare_short = _oracle_run(start, short, 77, False, 0.5), _oracle_run(fen_short, [], 77, False, 0.5)
    o_with_long, o_bare_long = _oracle_run(start, long, 80, False, 0.5), _oracle_run(fen_long, [], 80, False, 0.5)
    _check(with_short, o_with_short, "short, history")
    _check(bare_short, o_bare_short, "short, bare")
    _check(with_long, o_with_long, "long, history")
    _check(bare_long, o_bare_long, "long, bare")
    assert o_with_short["counts"] == o_bare_short["counts"]      # no fivefold within reach after seven moves
    assert o_with_long["counts"] != o_bare_long["counts"]
    # ... which the results show: another root value (the draws found on the way back) and other lines
    assert abs(o_with_long["root_q"] - o_bare_long["root_q"]) > 1e-3 and o_with_long["lines"] != o_bare_long["lines"]
    assert abs(with_long["root_q"] - bare_long["root_q"]) > 1e-3
    assert with_long["lines"] != bare_long["lines"]               # the q behind a move, a principal variation


def test_results_do_not_depend_on_the_slot():
    positions = _positions()
    ids = list(range(len(positions)))
    an = _ext(3, dirichlet=True)
    a = {r["id"]: r for r in an.analyse(positions, SIMS, ids=ids)}
    an.close()
    an = _ext(7, dirichlet=True)
    b = {r["id"]: r for r in an.analyse(positions[::-1], SIMS, ids=ids[::-1])}
    an.close()
    assert sorted(a) == sorted(b) == ids
    for i in ids:
        assert a[i] == b[i], (i, positions[i])              # every field, floats included: bit for bit


def _backend():
    from matrix0_amd.backend import M0Backend
    return M0Backend.from_state_dict(NET, net_ref.random_state_dict(NET, seed=7))


def test_fused_step_equals_split_step():
    from matrix0_amd import analysis
    positions = _positions()
    be = _backend()
    kw = dict(slots=5, multipv=MULTIPV, pv_len=PV_LEN, dirichlet=True)
    an = analysis.Analyzer(be, _cfg(), **kw)
    fused = an.analyse(positions, SIMS)
    st_f = an.stats()
    an.close()
    an = analysis.AnalyzerExt(be.infer_np, _cfg(), **kw)
    split = an.analyse(positions, SIMS)
    st_s = an.stats()
    an.close()
    be.close()
    assert len(fused) == len(split) == 30
    for f, s in zip(fused, split):
        assert f == s, f["fen"]
    assert st_f["evals"] == st_s["evals"] > 0 and st_f["sims"] == st_s["sims"]
    assert all(r["root_n"] == SIMS for r in fused if r["status"] == "ok")


def _host_policy(lg, idx):
    """Legal softmax in the engine's numerics: (logit - max) in float32, exp / sum / divide in float64, rounded to float32;
    uniform when the row holds a non-finite logit."""
    if not np.all(np.isfinite(lg)):
        return np.full(len(idx), 1.0 / len(idx), np.float32)
    sel = lg[idx].astype(np.float32)
    e = np.exp((sel - sel.max()).astype(np.float32).astype(np.float64))
    return (e / e.sum()).astype(np.float32)


def test_policy_mode_matches_the_host_softmax():
    from matrix0_amd import analysis, encoding
    rows = _fixture_rows()[:300]
    fens = [f for f, _ in rows]
    best = [m for _, m in rows]
    be = _backend()
    topk = 5
    an = analysis.Analyzer(be, _cfg(), slots=4, multipv=topk, pv_len=1)    # 4 * (8 + 1) = 36 rows a pass: 9 passes, the last ragged
    got = an.evaluate(fens, topk=topk)
    st = an.stats()
    an.close()
    planes, _, moves = encoding.encode_fens(fens)
    lg, val = be.infer_np(planes)
    be.close()
    assert st["evals"] == 300
    host = []
    for i, r in enumerate(got):
        ucis, idx = moves[i]
        pr = _host_policy(lg[i], idx)
        assert r["status"] == "ok" and r["nlegal"] == len(ucis) and r["root_n"] == 0 and r["evals"] == 1 and r["sims"] == 0, i
        assert np.float32(r["value"]).tobytes() == np.float32(val[i]).tobytes(), i
        assert len(r["lines"]) == min(topk, len(ucis)), i
        rep = [ln["prior"] for ln in r["lines"]]
        assert all(a >= b for a, b in zip(rep, rep[1:])), (i, rep)
        names = [ln["move"] for ln in r["lines"]]
        assert len(set(names)) == len(names)
        for ln in r["lines"]:
            k = ucis.index(ln["move"])
            assert ln["policy_index"] == idx[k] and ln["visits"] == 0 and ln["pv"] == [ln["move"]], i
            assert abs(ln["prior"] - float(pr[k])) <= 1e-6, (i, ln, float(pr[k]))
        rest = [float(pr[k]) for k, u in enumerate(ucis) if u not in names]
        if rest:
            assert max(rest) <= rep[-1] + 1e-6, (i, max(rest), rep[-1])
        order = sorted(range(len(ucis)), key=lambda k: (-float(pr[k]), k))[:topk]
        host.append({"lines": [{"move": ucis[k]} for k in order]})
    assert analysis.suite_accuracy(got, best) == analysis.suite_accuracy(host, best)


def test_mode_errors_leave_the_engine_usable():
    import ctypes as C
    from matrix0_amd import _lib, analysis
    from matrix0_amd import engine as eng
    L = _lib.lib()
    an = _ext(2)
    h = an.engine._h
    rec, res, rows = eng.GameRecord(), eng.AnalysisResult(), C.c_int(0)
    assert L.m0_selfplay_step(h, 1) == _lib.M0_ERR_STATE
    assert L.m0_selfplay_poll(h, C.byref(rec)) == _lib.M0_ERR_STATE
    assert L.m0_selfplay_ext_select(h, C.byref(rows), None, 0) == _lib.M0_ERR_STATE
    assert L.m0_selfplay_ext_expand(h, None, None, 0) == _lib.M0_ERR_STATE
    assert L.m0_search_begin(h, 0, ch.START_FEN.encode(), 8, 0, 1) == _lib.M0_ERR_STATE
    assert L.m0_search_select(h, C.byref(rows), None, 0) == _lib.M0_ERR_STATE
    assert "analysis engine" in _lib.last_error()
    # the other way round: a self-play engine refuses the analysis calls
    sp = eng.SelfplayEngine(None, eng.selfplay_cfg_from_dict(_cfg(), concurrent_games=2))
    assert L.m0_analysis_submit(sp._h, ch.START_FEN.encode(), None, 0, 8, 1) == _lib.M0_ERR_STATE
    assert L.m0_analysis_step(sp._h, 1) == _lib.M0_ERR_STATE
    assert L.m0_analysis_poll(sp._h, C.byref(res)) == _lib.M0_ERR_STATE
    assert L.m0_analysis_pending(sp._h) == _lib.M0_ERR_STATE
    sp.close()
    # creation refuses the table modes
    for key in ("tt_merge", "raw_legal_priors"):
        with pytest.raises(RuntimeError, match="M0_ERR_UNSUPPORTED"):
            analysis.AnalyzerExt(FakeNet(seed=3).infer_np, dict(_cfg(), engine={"compat": {key: True}}), slots=2)
    # bad submissions enqueue nothing
    with pytest.raises(ValueError, match="Illegal move"):
        an.engine.submit(ch.START_FEN, ["e2e4", "e2e4"], sims=SIMS, id=5)
    with pytest.raises(ValueError, match="FEN"):
        an.engine.submit("not a fen", [], sims=SIMS, id=6)
    with pytest.raises(RuntimeError):
        an.engine.submit(ch.START_FEN, [], sims=0, id=7)     # policy mode needs the engine's own network
    assert an.engine.pending() == 0 and an.engine.poll() is None
    # and the engine still works
    got = an.analyse([FENS[1], (ch.START_FEN, ["e2e4"])], SIMS, ids=[1, 9])
    an.close()
    _check(got[0], _oracle_set(False)[1], "after the errors")
    assert got[1]["status"] == "ok" and got[1]["root_n"] == SIMS and got[1]["lines"][0]["visits"] > 0


def test_every_entry_point_refuses_the_wrong_kind_of_engine():
    """One engine of each kind without a network, in the smallest configuration, and every entry point with otherwise valid
    arguments on the kinds that must refuse it: M0_ERR_STATE, no kernel launched, the engine untouched (stats unchanged, nothing
    pending).  m0_search_* on a match engine is accepted, as it always was.  The calls every kind accepts are checked too."""
    import ctypes as C
    from matrix0_amd import _lib
    from matrix0_amd import engine as eng
    L = _lib.lib()

    def cfg():
        return eng.selfplay_cfg_from_dict(_cfg(sims=4, leaves=2), concurrent_games=1)

    engines = {"self-play": eng.SelfplayEngine(None, cfg()), "match": eng.ArenaExtEngine(cfg()),
               "analysis": eng.AnalysisExtEngine(cfg())}
    cap = 1 * (2 + 1)
    pa, pb = np.zeros((cap, 19, 8, 8), np.float32), np.zeros((cap, 19, 8, 8), np.float32)
    lg, v = np.zeros((cap, 4672), np.float32), np.zeros(cap, np.float32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rows, rows_b, n, rn, fin, rq = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_double(0)
    rec, res, st = eng.GameRecord(), eng.AnalysisResult(), eng.SelfplayStats()
    fen = ch.START_FEN.encode()
    book = (C.c_char_p * 1)(fen)
    games, not_analysis = {"analysis"}, {"self-play", "match"}
    refused = [          # (call, the kinds that refuse it)
        ("m0_selfplay_step", lambda h: L.m0_selfplay_step(h, 1), games),
        ("m0_selfplay_poll", lambda h: L.m0_selfplay_poll(h, C.byref(rec)), games),
        ("m0_selfplay_set_openings", lambda h: L.m0_selfplay_set_openings(h, book, 1), games),
        ("m0_selfplay_ext_select", lambda h: L.m0_selfplay_ext_select(h, C.byref(rows), ptr(pa), cap), {"match", "analysis"}),
        ("m0_selfplay_ext_expand", lambda h: L.m0_selfplay_ext_expand(h, ptr(lg), ptr(v), 0), {"match", "analysis"}),
        ("m0_arena_ext_select", lambda h: L.m0_arena_ext_select(h, C.byref(rows), C.byref(rows_b), ptr(pa), ptr(pb), cap),
         {"self-play", "analysis"}),
        ("m0_arena_ext_expand", lambda h: L.m0_arena_ext_expand(h, ptr(lg), ptr(v), 0, ptr(lg), ptr(v), 0), {"self-play", "analysis"}),
        ("m0_search_begin", lambda h: L.m0_search_begin(h, 0, fen, 4, 0, 1), games),
        ("m0_search_select", lambda h: L.m0_search_select(h, C.byref(rows), ptr(pa), cap), games),
        ("m0_search_expand", lambda h: L.m0_search_expand(h, ptr(lg), ptr(v), 0), games),
        ("m0_search_result", lambda h: L.m0_search_result(h, 0, C.byref(n), None, None, None, None, None, C.byref(rq), C.byref(rn),
                                                          C.byref(fin)), games),
        ("m0_search_advance", lambda h: L.m0_search_advance(h, 0, 0, 4, 0), games),
        ("m0_analysis_submit", lambda h: L.m0_analysis_submit(h, fen, None, 0, 4, 1), not_analysis),
        ("m0_analysis_step", lambda h: L.m0_analysis_step(h, 1), not_analysis),
        ("m0_analysis_ext_select", lambda h: L.m0_analysis_ext_select(h, C.byref(rows), ptr(pa), cap), not_analysis),
        ("m0_analysis_ext_expand", lambda h: L.m0_analysis_ext_expand(h, ptr(lg), ptr(v), 0), not_analysis),
        ("m0_analysis_poll", lambda h: L.m0_analysis_poll(h, C.byref(res)), not_analysis),
        ("m0_analysis_pending", lambda h: L.m0_analysis_pending(h), not_analysis),
        ("m0_selfplay_set_tablebase", lambda h: L.m0_selfplay_set_tablebase(h, None, 0), {"match", "analysis"}),
    ]
    try:
        for kind, e in engines.items():
            before = e.stats()
            for name, call, kinds in refused:
                if kind not in kinds:
                    continue
                assert call(e._h) == _lib.M0_ERR_STATE, (name, kind)
                assert e.stats() == before, (name, kind)
                if kind == "analysis":
                    assert e.pending() == 0, name
            # what every kind accepts
            assert L.m0_selfplay_set_search_tablebase(e._h, None, 0) == _lib.M0_OK, kind
            assert L.m0_selfplay_stats_get(e._h, C.byref(st)) == _lib.M0_OK, kind
            assert L.m0_selfplay_running(e._h) in (0, 1), kind
            assert e.tb_leaves() == 0 and e.tb_adjudications() == 0, kind
            assert e.stats() == before, kind
        sp = engines["self-play"]
        assert L.m0_selfplay_set_tablebase(sp._h, None, 0) == _lib.M0_OK
        sp.search_begin(0, ch.START_FEN, 4, False, 1)             # and it still plays
        assert sp.search_select().shape[0] >= 1
    finally:
        for e in engines.values():
            e.close()
