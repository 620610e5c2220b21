"""The proof search on the GPU (include/m0_proof.h: csrc/tree_proof.h in select_kernel's proof instantiation and in
expand_kernel) against tests/proof_ref.py, through the split-step search with the hash evaluator of tests/hash_net.py.

Visit counts, move order, the rows of every pass, every root child's state and plies, the root's and the move must be identical
to the reference search; every state must be the exhaustive minimax's, whatever the reference says.  The engine's scan is the
reference's arithmetic in fp64 on the same float32 priors, but a children scan that the reference decides by less than 1e-4 is
not something to pin a test on: the game ids here were chosen, with the reference alone, so that no case has one and every
root is proven inside its budget, and every case asserts both.  The evaluator favours the forcing moves of the deeper positions
(HashNet's boost), or 64 simulations of a random evaluator would not find them."""
import functools

import numpy as np
import pytest

from oracle import chess_py as ch
from oracle import mcts_ref as ref
from tests import proof_ref as pr
from tests import tb_search_util as su
from tests import tb_util as tu
from tests.hash_net import HashNet
from tests.test_search_gpu import FENS, MCTS

pytestmark = pytest.mark.gpu

SEED = 1234
MIN_GAP = 1e-4                                                    # as tests/test_gumbel_gpu.py
CASES = [(64, 1), (64, 4), (200, 16)]                             # (simulations, leaves per pass)
# White's forcing moves in the positions that need more than one move found: (a position where the move is legal, the move)
WIN3, LOSS2, LOSS4 = pr.POSITIONS[1][0], pr.POSITIONS[3][0], pr.POSITIONS[4][0]
BOOST = {WIN3: [(WIN3, "a2a7"), (WIN3, "b1b8")],
         LOSS2: [("6k1/R7/8/8/8/8/8/1R5K w - - 0 1", "b1b8")],
         LOSS4: [("k7/8/1K6/8/8/8/8/7R w - - 0 1", "h1h8"), ("k7/8/1K6/8/8/8/8/7R w - - 0 1", "h1d1"),
                 ("1k6/8/1K6/8/8/8/8/3R4 w - - 0 1", "d1d8")]}
QUIET = FENS[3]
KQK_LOST = "8/8/8/4k3/8/8/8/KQ6 b - - 0 1"


def _net(fen):
    boost = [(ch.move_to_index(ch.Board(f), ch.Move.from_uci(u)), 4.0) for f, u in BOOST.get(fen, [])]
    return HashNet(seed=41, sharp=2.0, vscale=0.3, boost_white=boost)


def _uid(j, sims):
    return 5000 + 100 * j + (1 if j == 0 and sims == 64 else 0)


def _engine(G, L, sims, vl_active, proof=True, **cfg_kw):
    from matrix0_amd import engine as eng
    cfg = eng.selfplay_cfg_from_dict({"seed": SEED, "mcts": dict(MCTS, inference_batch_size=L), "selfplay": {"num_simulations": sims}},
                                     concurrent_games=G, virtual_loss_active=vl_active, **cfg_kw)
    e = eng.SelfplayEngine(None, cfg)
    if proof:
        e.set_proof()
    return e


def _run(e, net, G):
    """All searches to their end: the rows of every pass over all slots."""
    rows = []
    for _ in range(1000):
        planes = e.search_select()
        rows.append(int(planes.shape[0]))
        lg, v = net.infer_np(planes) if planes.shape[0] else (np.zeros((0, 4672), np.float32), np.zeros((0,), np.float32))
        e.search_expand(lg, v)
        if all(e.search_result(g)["finished"] for g in range(G)):
            break
    return rows


@functools.lru_cache(maxsize=None)
def reference(j, sims, L, vl):
    """The reference search of position j in one case, computed once."""
    fen = pr.POSITIONS[j][0]
    cfg = ref.MCTSConfig.from_dict(dict(MCTS, inference_batch_size=L, use_tt=False, virtual_loss_active=vl, numerics="engine"))
    o = pr.ProofMCTS(cfg, _net(fen).infer_np, seed=SEED, game=_uid(j, sims))
    return o, o.search(ch.Board(fen), sims)


@functools.lru_cache(maxsize=None)
def engine_search(j, sims, L, vl):
    """The engine's search of position j in one case: (result, proof result, rows of every pass, evaluations)."""
    fen = pr.POSITIONS[j][0]
    e = _engine(1, L, sims, vl)
    e.search_begin(0, fen, sims, False, _uid(j, sims))
    rows = _run(e, _net(fen), 1)
    out = e.search_result(0), e.search_proof_result(0), rows, int(e.stats()["evals"])
    e.close()
    return out


@pytest.mark.parametrize("vl", [True, False])
@pytest.mark.parametrize("sims,L", CASES)
@pytest.mark.parametrize("j", range(len(pr.POSITIONS)))
def test_tree_and_proofs_match_the_reference(j, sims, L, vl):
    o, want = reference(j, sims, L, vl)
    assert o.min_gap >= MIN_GAP, f"a children scan decided by {o.min_gap}: choose another game id for this case"
    assert want["state"] != pr.NONE and o.sims <= sims, "the reference does not prove this root: choose another game id"
    res, pres, rows, evals = engine_search(j, sims, L, vl)
    kids = list(want["root"].children.values())
    assert res["finished"] and res["moves"] == [c.move.uci() for c in kids]
    assert res["n"].tolist() == [c.n for c in kids], (res["n"].tolist(), [c.n for c in kids])
    assert res["root_n"] == want["root"].n == o.sims
    assert rows == o.rows, (rows, o.rows)
    assert evals == o.evals
    np.testing.assert_allclose(res["prior"], [c.prior for c in kids], rtol=0, atol=1e-6)
    np.testing.assert_allclose(res["q"], [c.q for c in kids], rtol=0, atol=1e-9)
    assert list(zip(pres["child_state"], pres["child_plies"].tolist())) == want["children"]
    assert (pres["state"], pres["plies"]) == (want["state"], want["plies"])
    assert pres["pick"] == want["pick"]


@functools.lru_cache(maxsize=None)
def quiet_reference(L):
    cfg = ref.MCTSConfig.from_dict(dict(MCTS, inference_batch_size=L, use_tt=False, virtual_loss_active=True, numerics="engine"))
    o = pr.ProofMCTS(cfg, _net(QUIET).infer_np, seed=SEED, game=6000)
    return o, o.search(ch.Board(QUIET), 64)


@pytest.mark.parametrize("G", [2, 3, 4])
def test_slots_side_by_side_end_one_by_one(G):
    """Searches that are proven after different numbers of passes, and one that never is, share the launches: a finished
    slot stays finished and costs nothing more.  (The positions without favoured moves: one evaluator for all slots.)"""
    sims, L = 64, 1
    want = ([reference(j, sims, L, True) for j in (0, 2, 5)] + [quiet_reference(L)])[4 - G:]
    fens = ([pr.POSITIONS[j][0] for j in (0, 2, 5)] + [QUIET])[4 - G:]
    uids = ([_uid(j, sims) for j in (0, 2, 5)] + [6000])[4 - G:]
    e = _engine(G, L, sims, True)
    for g in range(G):
        e.search_begin(g, fens[g], sims, False, uids[g])
    rows = _run(e, _net(None), G)
    n = max(len(o.rows) for o, _ in want)
    assert rows == [sum(o.rows[p] for o, _ in want if p < len(o.rows)) for p in range(n)]
    for g, (o, w) in enumerate(want):
        res, pres = e.search_result(g), e.search_proof_result(g)
        kids = list(w["root"].children.values())
        assert res["n"].tolist() == [c.n for c in kids], g
        assert (pres["state"], pres["plies"], pres["pick"]) == (w["state"], w["plies"], w["pick"]), g
        assert list(zip(pres["child_state"], pres["child_plies"].tolist())) == w["children"], g
    assert int(e.stats()["evals"]) == sum(o.evals for o, _ in want)
    e.close()


@pytest.mark.parametrize("sims,L", CASES)
@pytest.mark.parametrize("j", range(len(pr.POSITIONS)))
def test_every_reported_state_is_the_minimax_value(j, sims, L):
    """Without the reference search: the positions are small enough to solve."""
    fen, state, plies, nlegal = pr.POSITIONS[j]
    res, pres, _, _ = engine_search(j, sims, L, True)
    assert len(res["moves"]) == nlegal
    # a distance is that of the first proof found: never below the shortest, and exact where only one line proves it
    assert pres["state"] == state and pres["plies"] >= plies and (pres["plies"] - plies) % 2 == 0
    if plies <= 1:
        assert pres["plies"] == plies
    assert int(res["n"].sum()) < sims, "a search whose root is proven ends"
    board = ch.Board(fen)
    for mv, cs, cp in zip(res["moves"], pres["child_state"], pres["child_plies"].tolist()):
        if cs == pr.NONE:
            continue
        b = board.copy()
        b.push(ch.Move.from_uci(mv))
        true_state, true_plies = pr.solve(b.fen(), max(cp, 3))
        assert true_state == cs and true_plies <= cp, (fen, mv, (cs, cp), (true_state, true_plies))
    picked = (pres["child_state"][pres["pick"]], int(pres["child_plies"][pres["pick"]]))
    if state == pr.WIN:
        assert picked == (pr.LOSS, pres["plies"] - 1)
    elif state == pr.LOSS:
        assert picked == (pr.WIN, pres["plies"] - 1)
    else:
        assert picked == (pr.DRAW, 0)


@pytest.mark.parametrize("L", [1, 4, 16])
def test_a_quiet_position_is_searched_as_without_the_mode(L):
    sims, uid = 64, 6000
    o, want = quiet_reference(L)
    assert not o.proofs and o.sims == sims, "the reference proves something here: choose another position"
    got = []
    for proof in (True, False):
        e = _engine(1, L, sims, True, proof=proof)
        e.search_begin(0, QUIET, sims, False, uid)
        rows = _run(e, _net(QUIET), 1)
        got.append((e.search_result(0), rows, int(e.stats()["evals"])))
        if proof:
            pres = e.search_proof_result(0)
            assert pres["state"] == pr.NONE and set(pres["child_state"]) == {pr.NONE}
            assert pres["pick"] == int(np.argmax(got[0][0]["n"]))
        e.close()
    (a, rows_a, evals_a), (b, rows_b, evals_b) = got
    assert rows_a == rows_b and evals_a == evals_b and a["moves"] == b["moves"]
    for key in ("n", "idx", "prior", "q"):
        assert np.array_equal(a[key], b[key]), key
    assert a["root_q"] == b["root_q"] and a["root_n"] == b["root_n"] == sims


@pytest.fixture(scope="module")
def tb3():
    from matrix0_amd.tablebase import Tablebase
    tb = Tablebase.build(3, 0)
    yield tb
    tb.close()


@pytest.mark.parametrize("L", [1, 4, 16])
def test_table_hits_prove_a_root_with_the_tables_distance(tb3, L):
    """K and Q against K with the lone king to move: every reply is a hit, the root is lost in the table's distance."""
    board = ch.Board(KQK_LOST)
    wdl, dtm = su.lookup(su.men_of(board), board.turn, tu.ref_tables())
    assert wdl == -1 and dtm > 2
    e = _engine(1, L, 64, True)
    e.set_search_tablebase(tb3, 3)
    e.search_begin(0, KQK_LOST, 64, False, 6100)
    rows = _run(e, _net(KQK_LOST), 1)
    res, pres, leaves = e.search_result(0), e.search_proof_result(0), e.tb_leaves()
    e.close()
    assert res["finished"] and (pres["state"], pres["plies"]) == (pr.LOSS, dtm)
    kids = su.ranked_moves(board, tu.ref_tables())
    by_move = {m.uci(): (w, d) for m, w, d in kids}
    for mv, cs, cp in zip(res["moves"], pres["child_state"], pres["child_plies"].tolist()):
        assert (cs, cp) == (pr.WIN, by_move[mv][1]) and by_move[mv][0] == 1, mv
    assert int(pres["child_plies"][pres["pick"]]) == dtm - 1
    # one visit per reply, none evaluated: the root's own evaluation is all the network saw
    assert sum(rows) == 1 and leaves == len(kids) == int(res["n"].sum())


@pytest.mark.parametrize("L", [1, 4, 16])
def test_a_kept_subtree_keeps_its_proofs(L):
    j, sims = 1, 200                                                # WIN 3
    fen = pr.POSITIONS[j][0]
    e = _engine(1, L, sims, True)
    e.search_begin(0, fen, sims, False, _uid(j, sims))
    _run(e, _net(fen), 1)
    pres = e.search_proof_result(0)
    assert pres["state"] == pr.WIN
    plies, evals = pres["plies"], int(e.stats()["evals"])
    for want_state in (pr.LOSS, pr.WIN):                            # after the move, then after the reply
        e.search_advance(0, pres["pick"], sims, False)
        planes = e.search_select()
        assert planes.shape[0] == 0
        e.search_expand(np.zeros((0, 4672), np.float32), np.zeros((0,), np.float32))
        res, pres = e.search_result(0), e.search_proof_result(0)
        plies -= 1
        assert res["finished"] and (pres["state"], pres["plies"]) == (want_state, plies)
        assert int(e.stats()["evals"]) == evals, "a root that is proven when the search starts costs no evaluation"
        assert 0 <= pres["pick"] < len(res["moves"])
    e.close()


def test_the_setter_says_when_and_where_it_cannot_be_used():
    from matrix0_amd import engine as eng
    from matrix0_amd.backend import M0Backend
    from oracle import net_ref
    base = {"seed": 1, "mcts": dict(MCTS, inference_batch_size=8), "selfplay": {"num_simulations": 8}}
    cfg = eng.selfplay_cfg_from_dict(base, concurrent_games=1)
    e = eng.SelfplayEngine(None, cfg)
    with pytest.raises(RuntimeError, match="not set"):
        e.search_proof_result(0)
    e.set_proof()
    e.set_proof(False)
    e.set_proof(True)                                               # again, before the first search: the last one holds
    with pytest.raises(ValueError, match="proof search"):
        e.set_gumbel()
    e.search_begin(0, ch.START_FEN, 8, False, 0)
    assert e.search_proof_result(0)["pick"] == -1                   # not finished
    with pytest.raises(RuntimeError, match="before the first"):
        e.set_proof()
    e.close()
    e = eng.SelfplayEngine(None, cfg)
    e.set_gumbel()
    with pytest.raises(ValueError, match="Gumbel"):
        e.set_proof()
    e.close()
    e = eng.SelfplayEngine(None, eng.selfplay_cfg_from_dict(base, concurrent_games=1, compat={"tt_merge": True}))
    with pytest.raises(ValueError, match="tt_merge"):
        e.set_proof()
    e.close()
    net = dict(planes=19, channels=32, blocks=1, attention_heads=2, policy_size=4672, norm="group", activation="silu",
               preact=True, policy_factor_rank=16, self_supervised=False)
    be = M0Backend.from_state_dict(net, net_ref.random_state_dict(net, seed=1))
    e = eng.SelfplayEngine(be, cfg)
    with pytest.raises(RuntimeError, match="own network"):
        e.set_proof()
    e.close()
    be.close()
    for other in (eng.ArenaExtEngine(cfg), eng.AnalysisExtEngine(cfg)):      # match and analysis engines take the mode
        other.set_proof()
        other.close()


def test_a_match_engine_plays_the_proven_move():
    """engine.proof_search in matches: from a book of won positions every game is the forced mate, move by move (each move a
    fresh search: the side to move proves its win and plays the shortest, the loser its longest defence)."""
    from matrix0_amd import engine as eng
    book = [pr.POSITIONS[0][0], WIN3]
    cfg = eng.selfplay_cfg_from_dict({"seed": 21, "mcts": dict(MCTS, inference_batch_size=8, dirichlet_frac=0.0),
                                      "selfplay": {"num_simulations": 200, "max_game_len": 10, "opening_random_plies": 0,
                                                   "resign_threshold": -2.0, "min_resign_plies": 10 ** 9}},
                                     concurrent_games=3, total_games=8, record_games=False)
    cfg.arena_paired_openings = 1
    e = eng.ArenaExtEngine(cfg)
    e.set_openings(book)
    e.set_proof()
    net = _net(WIN3)
    z0 = (np.zeros((0, 4672), np.float32), np.zeros((0,), np.float32))
    recs = []
    for _ in range(5000):
        if not e.running():
            break
        pa, pb = e.arena_ext_select()
        la, va = net.infer_np(pa) if pa.shape[0] else z0
        lb, vb = net.infer_np(pb) if pb.shape[0] else z0
        e.arena_ext_expand(la, va, lb, vb)
        while (r := e.poll()) is not None:
            recs.append(r)
    evals = int(e.stats()["evals"])
    assert not e.running() and len(recs) == 8
    e.close()
    plies = 0
    for r in recs:
        want = {book[0]: 1, book[1]: 3}[r["start_fen"]]
        assert len(r["played"]) == want and r["result"] == 1.0 and not r["draw"], r
        assert ch.Board(eng.fen_after(r["start_fen"], r["played"])).is_checkmate(), r
        plies += want
    assert evals < plies * 200, "searches that prove their root end before their budget"


# ---- analysis engine and UCI (include/m0_proof.h: m0_analysis_last_proof, the proof ranking of analysis_lines_kernel)
def _analysis_engine(sims, L, proof=True, multipv=8, pv_len=16):
    from matrix0_amd import engine as eng
    cfg = eng.selfplay_cfg_from_dict({"seed": SEED, "mcts": dict(MCTS, inference_batch_size=L, dirichlet_frac=0.0),
                                      "selfplay": {"num_simulations": sims}}, concurrent_games=1, virtual_loss_active=True)
    e = eng.AnalysisExtEngine(cfg, multipv=multipv, pv_len=pv_len)
    if proof:
        e.set_proof()
    return e


def _ranked(root, proofs):
    """The root children of the reference in the proof ranking: (index, line state, line plies) best first."""
    kids = list(root.children.values())

    def key(i):
        s, p = proofs[i]
        return (2, -p) if s == pr.LOSS else ((0, p) if s == pr.WIN else (1, kids[i].n))
    order = sorted(range(len(kids)), key=lambda i: (tuple(-x for x in key(i)), i))
    flip = {pr.LOSS: pr.WIN, pr.WIN: pr.LOSS, pr.DRAW: pr.DRAW, pr.NONE: pr.NONE}
    return [(i, flip[proofs[i][0]], proofs[i][1] + 1 if proofs[i][0] in (pr.WIN, pr.LOSS) else 0) for i in order]


@pytest.mark.parametrize("L", [1, 4, 16])
def test_the_analysis_engine_reports_and_ranks_proofs(L):
    """WIN 3: the first line is the mate, `proof` win in 3 plies, its variation the three moves of the mate; the lines are
    ranked as the reference's tree ranks them; the search spends fewer nodes than it was given."""
    sims, uid = 200, _uid(1, 200)
    cfg = ref.MCTSConfig.from_dict(dict(MCTS, inference_batch_size=L, use_tt=False, virtual_loss_active=True, numerics="engine",
                                        dirichlet_frac=0.0))
    o = pr.ProofMCTS(cfg, _net(WIN3).infer_np, seed=SEED, game=uid)
    want = o.search(ch.Board(WIN3), sims)
    assert want["state"] == pr.WIN and o.min_gap >= MIN_GAP
    e = _analysis_engine(sims, L)
    e.submit(WIN3, sims=sims, id=uid)
    net = _net(WIN3)
    for _ in range(300):
        e.step(net.infer_np, 1)
        r = e.poll()
        if r is not None:
            break
    e.close()
    assert r["status"] == "ok" and r["root_n"] == o.sims < sims == r["sims"]
    assert (r["proof"], r["proof_plies"]) == (pr.WIN, want["plies"]) and want["plies"] == 3
    kids = list(want["root"].children.values())
    ranked = _ranked(want["root"], want["children"])[:8]
    assert [ln["move"] for ln in r["lines"]] == [kids[i].move.uci() for i, _, _ in ranked]
    assert [(ln["proof"], ln["proof_plies"]) for ln in r["lines"]] == [(s, p) for _, s, p in ranked]
    assert [ln["visits"] for ln in r["lines"]] == [kids[i].n for i, _, _ in ranked]
    best = r["lines"][0]
    assert (best["proof"], best["proof_plies"]) == (pr.WIN, 3) and ranked[0][0] == want["pick"]
    assert len(best["pv"]) == 3
    assert ch.Board(__import__("matrix0_amd.engine", fromlist=["x"]).fen_after(WIN3, best["pv"])).is_checkmate()


def test_an_analysis_engine_without_the_mode_answers_as_before():
    sims, L = 64, 4
    got = []
    for proof in (False, True):
        e = _analysis_engine(sims, L, proof=proof)
        e.submit(QUIET, sims=sims, id=6000)
        net = _net(QUIET)
        r = None
        for _ in range(100):
            e.step(net.infer_np, 1)
            r = e.poll()
            if r is not None:
                break
        e.close()
        got.append(r)
    off, on = got
    assert "proof" not in off and on["proof"] == pr.NONE and all(ln["proof"] == pr.NONE for ln in on["lines"])
    for ln in on["lines"]:
        del ln["proof"], ln["proof_plies"]
    del on["proof"], on["proof_plies"]
    assert on == off                                  # nothing proven: the ranking by visits, the most visited variations


def _uci_on(engine, net, sims):
    from matrix0_amd import uci
    out = []
    u = uci.UciEngine(engine, {"selfplay": {"num_simulations": sims}, "mcts": {"inference_batch_size": 4}}, out=out.append,
                      step=lambda: engine.step(net.infer_np, 1))
    return u, out


def test_uci_prints_score_mate_and_honours_go_mate():
    sims = 200
    e = _analysis_engine(sims, 4)
    u, out = _uci_on(e, _net(WIN3), sims)
    u.command("setoption name ProveMates value true")
    u.dirty = False                                   # this engine already runs the mode
    u.command(f"position fen {WIN3}")
    u.command("go nodes 200")
    n = 0
    while u.pump():
        n += 1
        assert n < 300
    info = [o for o in out if o.startswith("info depth") and " multipv 1 " in o][-1]
    assert " score mate 2 " in info and len(info.split(" pv ")[1].split()) == 3, info
    nodes = int(info.split(" nodes ")[1].split()[0])
    assert 0 < nodes < sims
    assert out[-1].startswith("bestmove " + info.split(" pv ")[1].split()[0])
    # go mate 2 from a fresh tree: not ignored, and over before the budget
    out.clear()
    u.command("ucinewgame")
    u.command("go mate 2")
    assert not any("ignored" in o for o in out)
    n = 0
    while u.pump():
        n += 1
        assert n < 300
    info = [o for o in out if o.startswith("info depth") and " multipv 1 " in o][-1]
    assert " score mate 2 " in info and int(info.split(" nodes ")[1].split()[0]) < sims
    # the next search of the position after the mating line's first two moves starts in the held tree, proven: no evaluation
    pv = info.split(" pv ")[1].split()
    evals = int(e.stats()["evals"])
    out.clear()
    u.command(f"position fen {WIN3} moves {pv[0]} {pv[1]}")
    u.command("go nodes 200")
    while u.pump():
        pass
    assert any(" score mate 1 " in o for o in out) and out[-1] == f"bestmove {pv[2]}"
    assert int(e.stats()["evals"]) == evals
    e.close()
