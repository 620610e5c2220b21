"""The endgame tablebases inside the search, on the GPU: the probe of select_kernel against an oracle MCTS that treats a
table hit as a terminal leaf (over the independent generator's tables), an attached set that can never hit, the match engine
adjudicating from the tables, and the analysis engine answering table roots on the host.

The parity roots are 4-man positions, so the root is never a hit at max_pieces = 3.  For each of them but one the oracle was
checked (on the CPU, when the FENs were picked) to meet at least 10 table leaves and at least 10 network leaves in every run
below; `test_oracle_meets_both_kinds_of_leaves` asserts it again.  The exception is the KBKN root: every 3-man position it can
reach is KBK, KNK or KK, which the insufficient-material test -- ahead of the probe, as specified -- ends first, so no KBKN
root can meet a table leaf at all.  The root is kept and the oracle's count for it is asserted to be zero; the draw_penalty
path of a table draw is taken from the KRKP and KPKP roots, whose captures lead into KPK and KRK draws."""
import functools

import numpy as np
import pytest

from oracle import chess_py as ch
from oracle import mcts_ref as ref
from tests import tb_search_util as su
from tests import tb_util as tu
from tests.fake_net import FakeNet
from tests.hash_net import HashNet
from tests.test_search_gpu import MCTS

KQKR = "7K/8/8/7r/8/8/6k1/3Q4 w - - 0 1"
KBKN = "8/8/8/3k4/8/2n5/3B4/4K3 w - - 0 1"
ROOTS = [KQKR,
         tu.flip_fen(KQKR),                               # Black to move and the greater side: the device-side flip
         "8/8/8/8/k7/8/5p1R/4K3 w - - 0 1",               # KRKP
         KBKN,
         "8/6k1/8/8/2pK4/1P6/8/8 w - - 0 1"]              # KPKP, bxc4 available
RIGHT_LEFT = "4k3/8/8/8/8/8/8/R3K3 w Q - 0 1"             # no hit (a right is left); every child is one
SIMS = 128
RUNS = [(8, True), (96, True), (8, False), (96, False)]   # leaves per pass, virtual loss


class TbMCTS(ref.MCTS):
    """The oracle with the tables: a leaf is terminal when the game is over or when it is a hit in `tables`; a hit is worth
    +1 / -1 for the side to move, draw_penalty for a table draw."""

    def __init__(self, *a, tables=None, max_men=3, **kw):
        super().__init__(*a, **kw)
        self.tables, self.max_men, self.tb_leaves, self.net_leaves = tables, max_men, 0, 0

    def run_batched(self, board, root, sims):
        L = int(self.cfg.inference_batch_size) or 96
        done = 0
        while done < sims:
            batch_n = min(L, sims - done)
            inflight = {} if self.cfg.virtual_loss_active else None
            samples = []
            for _ in range(batch_n):
                node, path, leaf = self.select(board.copy(), root, inflight)
                hit = None if leaf.is_game_over() else su.py_probe(leaf, self.tables, self.max_men)
                if leaf.is_game_over():
                    self.backpropagate(path, self.terminal_value(leaf))
                elif hit is not None:
                    self.tb_leaves += 1
                    self.backpropagate(path, float(hit[0]) if hit[0] else float(self.cfg.draw_penalty))
                else:
                    samples.append((node, list(path), leaf))
            if samples:
                x = np.stack([ch.encode_board(b) for (_, _, b) in samples], axis=0)
                pol, val = self.infer_np(x)
                self.evals += len(samples)
                self.net_leaves += len(samples)
                for (node, path, leaf), p, v in zip(samples, pol, val):
                    if not node.expanded:
                        self.expand(node, leaf, p)
                        self.register_children(node, leaf)
                    self.backpropagate(path, float(np.clip(v, -1.0, 1.0)))
            done += batch_n


@functools.lru_cache(maxsize=None)
def oracle_run(fen, uid, L, vl_active, dirichlet=False, sims=SIMS):
    """One oracle search with the reference generator's tables (computed once per argument set, never modified)."""
    m = dict(MCTS, inference_batch_size=L)
    cfg = ref.MCTSConfig.from_dict(dict(m, use_tt=False, virtual_loss_active=vl_active, dirichlet_plies=(30 if dirichlet else 0),
                                        numerics="engine"))
    o = TbMCTS(cfg, FakeNet(seed=3, sharp=8.0).infer_np, seed=1234, game=uid, tables=tu.ref_tables())
    _, _, rq = o.run(ch.Board(fen), num_simulations=sims, ply=0)
    return o, rq


@pytest.mark.parametrize("L,vl_active", RUNS)
def test_oracle_meets_both_kinds_of_leaves(L, vl_active):
    for g, fen in enumerate(ROOTS):
        o, _ = oracle_run(fen, 300 + g, L, vl_active)
        print(f"L={L} vl={vl_active} {fen}: {o.tb_leaves} table leaves, {o.net_leaves} network leaves, {o.evals} evaluations")
        assert su.py_probe(ch.Board(fen), tu.ref_tables()) is None
        assert o.net_leaves >= 10, fen
        if fen == KBKN:
            assert o.tb_leaves == 0, fen                 # insufficient material comes first (see the module docstring)
        else:
            assert o.tb_leaves >= 10, fen


# ---------------------------------------------------------------- GPU ----------------------------------------------------------------
@pytest.fixture(scope="module")
def tb3():
    from matrix0_amd.tablebase import Tablebase
    tb = Tablebase.build(3, 0)
    yield tb
    tb.close()


def _search_engine(G, L, vl_active, tb, max_pieces=3):
    from matrix0_amd import engine as eng
    cfg = eng.selfplay_cfg_from_dict({"seed": 1234, "mcts": dict(MCTS, inference_batch_size=L), "selfplay": {"num_simulations": SIMS}},
                                     concurrent_games=G, virtual_loss_active=vl_active)
    e = eng.SelfplayEngine(None, cfg)
    if tb is not None:
        e.set_search_tablebase(tb, max_pieces)
    return e


def _run_search(e, net, G):
    for _ in range(10000):
        planes = e.search_select()
        lg, v = net.infer_np(planes) if planes.shape[0] else (np.zeros((0, 4672), np.float32), np.zeros((0,), np.float32))
        e.search_expand(lg, v)
        if all(e.search_result(g)["finished"] for g in range(G)):
            break
    return [e.search_result(g) for g in range(G)]


def _compare(res, o, rq, tag):
    kids = list(o._last_root.children.values())
    assert res["finished"] and res["moves"] == [c.move.uci() for c in kids], tag
    assert res["idx"].tolist() == [c.move_idx for c in kids], tag
    assert res["n"].tolist() == [c.n for c in kids], (tag, res["n"].tolist(), [c.n for c in kids])
    np.testing.assert_allclose(res["prior"], [c.prior for c in kids], rtol=0, atol=1e-6, err_msg=str(tag))
    np.testing.assert_allclose(res["q"], [c.q for c in kids], rtol=0, atol=1e-9, err_msg=str(tag))
    assert abs(res["root_q"] - rq) <= 1e-9 and res["root_n"] == o._last_root.n, tag


@pytest.mark.gpu
@pytest.mark.parametrize("L,vl_active", RUNS)
def test_search_with_tables_matches_the_oracle(tb3, L, vl_active):
    G = len(ROOTS)
    e = _search_engine(G, L, vl_active, tb3)
    for g, fen in enumerate(ROOTS):
        e.search_begin(g, fen, SIMS, False, 300 + g)
    results = _run_search(e, FakeNet(seed=3, sharp=8.0), G)
    evals, leaves = int(e.stats()["evals"]), e.tb_leaves()
    e.close()
    want = [oracle_run(fen, 300 + g, L, vl_active) for g, fen in enumerate(ROOTS)]
    print(f"L={L} vl={vl_active}: {evals} evaluations, {leaves} table leaves; oracle {[(o.evals, o.tb_leaves) for o, _ in want]}")
    for g, (o, rq) in enumerate(want):
        _compare(results[g], o, rq, (L, vl_active, ROOTS[g]))
    assert evals == sum(o.evals for o, _ in want)
    assert leaves == sum(o.tb_leaves for o, _ in want)


@pytest.mark.gpu
def test_root_with_a_castling_right_is_searched_and_every_child_is_a_hit(tb3):
    e = _search_engine(1, 8, True, tb3)
    e.search_begin(0, RIGHT_LEFT, SIMS, False, 77)
    res = _run_search(e, FakeNet(seed=3, sharp=8.0), 1)[0]
    evals, leaves = int(e.stats()["evals"]), e.tb_leaves()
    e.close()
    o, rq = oracle_run(RIGHT_LEFT, 77, 8, True)
    _compare(res, o, rq, RIGHT_LEFT)
    assert (o.evals, o.tb_leaves) == (1, SIMS)             # the root's own evaluation and nothing else
    assert (evals, leaves) == (1, SIMS)


BOOK3 = ["8/8/8/4k3/8/8/8/KQ6 w - - 0 1", "8/8/8/4k3/8/8/8/KR6 w - - 0 1", "8/8/8/4K3/8/8/8/kq6 b - - 0 1", "8/8/8/8/8/k7/P7/K7 w - - 0 1"]
PLAY_MCTS = {"cpuct": 2.5, "dirichlet_plies": 30, "selection_jitter": 0.05, "fpu_reduction": 0.1, "draw_penalty": -0.05,
             "legal_softmax": True, "inference_batch_size": 4}


def _selfplay(tb, games=8, max_game_len=6):
    from matrix0_amd import engine as eng
    cfg = eng.selfplay_cfg_from_dict({"seed": 11, "mcts": PLAY_MCTS,
                                      "selfplay": {"num_simulations": 8, "max_game_len": max_game_len, "opening_random_plies": 0}},
                                     concurrent_games=games, total_games=games)
    e = eng.SelfplayEngine(None, cfg)
    e.set_openings(BOOK3)
    if tb is not None:
        e.set_search_tablebase(tb, 2)
    net, recs = HashNet(seed=5, sharp=8.0), []
    for _ in range(20000):
        if not e.running():
            break
        planes = e.ext_select()
        lg, v = net.infer_np(planes) if planes.shape[0] else (np.zeros((0, 4672), np.float32), np.zeros((0,), np.float32))
        e.ext_expand(lg, v)
        while (r := e.poll()) is not None:
            recs.append(r)
    assert not e.running()
    out = (sorted(recs, key=lambda r: r["game_index"]), int(e.stats()["evals"]), e.tb_leaves(), e.tb_adjudications())
    e.close()
    return out


@pytest.mark.gpu
def test_an_attached_set_that_cannot_hit_changes_nothing(tb3):
    """max_pieces = 2: only KK is in reach, and inside the search the insufficient-material test ends it first, so no leaf
    comes from the tables.  After a played move the host probe comes before the game-over test, exactly as with
    m0_selfplay_set_tablebase: a game that reaches KK is counted as adjudicated, with the draw it would have had anyway."""
    a, evals_a, leaves_a, _ = _selfplay(tb3)
    b, evals_b, leaves_b, adj_b = _selfplay(None)
    assert len(a) == len(b) == 8 and evals_a == evals_b and (leaves_a, leaves_b, adj_b) == (0, 0, 0)
    for x, y in zip(a, b):
        for k in ("game_index", "moves", "resigned", "resigner", "draw", "result", "played", "start_fen"):
            assert x[k] == y[k], k
        for k in ("s", "pi", "z", "legal_mask", "search_values", "played_raw"):
            assert x[k].tobytes() == y[k].tobytes(), k


FORCED_W, FORCED_P = "8/8/8/8/8/8/r1k5/K6Q w - - 0 1", "8/8/8/8/8/7P/r1k5/K7 w - - 0 1"      # Kxa2 is the only legal move
BOOK4 = [FORCED_W,                                        # ... into KQK, won
         tu.flip_fen(FORCED_W),                           # the same with Black to move and the greater side
         FORCED_P,                                        # ... into KPK
         "8/8/4k3/8/3r4/8/3Q4/4K3 w - - 0 1"]             # nothing forced: the rook hangs


def _match(tb, slots, games=8):
    from matrix0_amd import _lib, engine as eng
    cfg = eng.selfplay_cfg_from_dict({"seed": 21, "mcts": dict(PLAY_MCTS, inference_batch_size=8),
                                      "selfplay": {"num_simulations": 32, "max_game_len": 10, "opening_random_plies": 0,
                                                   "resign_threshold": -2.0, "min_resign_plies": 10 ** 9}},
                                     concurrent_games=slots, total_games=games, record_games=False)
    cfg.arena_paired_openings = 1
    e = eng.ArenaExtEngine(cfg)
    e.set_openings(BOOK4)
    assert e._L.m0_selfplay_set_tablebase(e._h, tb.handle, 3) == _lib.M0_ERR_STATE      # the old call: self-play engines only
    e.set_search_tablebase(tb, 3)
    na, nb = HashNet(seed=5, sharp=8.0), HashNet(seed=6, sharp=8.0)
    z0 = (np.zeros((0, 4672), np.float32), np.zeros((0,), np.float32))
    recs = []
    for _ in range(20000):
        if not e.running():
            break
        pa, pb = e.arena_ext_select()
        la, va = na.infer_np(pa) if pa.shape[0] else z0
        lb, vb = nb.infer_np(pb) if pb.shape[0] else z0
        e.arena_ext_expand(la, va, lb, vb)
        while (r := e.poll()) is not None:
            recs.append(r)
    assert not e.running()
    out = (sorted(recs, key=lambda r: r["game_index"]), e.tb_adjudications(), e.tb_leaves())
    e.close()
    return out


@pytest.mark.gpu
def test_match_engine_adjudicates_from_the_tables(tb3):
    from matrix0_amd import engine as eng
    recs, adjudicated, leaves = _match(tb3, 2)
    assert len(recs) == 8 and leaves > 0
    reached = 0
    for r in recs:
        fens = [eng.fen_after(r["start_fen"], r["played"][:k]) for k in range(1, len(r["played"]) + 1)]
        men = [sum(c.isalpha() for c in f.split()[0]) for f in fens]
        assert all(n == 4 for n in men[:-1]), r                   # a game that reaches three men ends there
        if men and men[-1] <= 3:
            hit, wdl, _ = tb3.probe([fens[-1]])
            assert hit[0], fens[-1]
            white = fens[-1].split()[1] == "w"
            assert r["result"] == float(wdl[0]) * (1.0 if white else -1.0) and r["draw"] == (wdl[0] == 0), (r, fens[-1])
            reached += 1
    print(f"{reached} of {len(recs)} games reached a 3-man position; {adjudicated} adjudicated, {leaves} table leaves")
    forced = [r for r in recs if r["start_fen"] != BOOK4[3]]
    assert all(len(r["played"]) == 1 for r in forced) and len(forced) >= 1        # the one legal move, then the verdict
    assert adjudicated == reached and reached >= len(forced)
    again, adjudicated2, leaves2 = _match(tb3, 2)
    wide, adjudicated5, _ = _match(tb3, 5)
    for other in (again, wide):
        assert [(r["game_index"], r["start_fen"], r["played"], r["result"]) for r in other] == \
               [(r["game_index"], r["start_fen"], r["played"], r["result"]) for r in recs]
    assert (adjudicated2, leaves2, adjudicated5) == (adjudicated, leaves, adjudicated)


MULTIPV, PV_LEN = 3, 8
TABLE_ROOTS = ["7k/8/6K1/8/8/8/8/5Q2 w - - 0 1",          # mate in one
               "8/8/8/4k3/8/8/4K3/R7 w - - 0 1",          # a long rook win: the line is cut at pv_len
               "8/8/8/3k4/8/8/1q6/7K w - - 0 1",          # lost, Black the greater side
               "8/8/8/8/8/k7/P7/K7 w - - 0 1",            # a drawn pawn ending
               "8/8/8/4k3/8/8/8/KQ6 b - - 0 1",           # the loser to move
               "4k3/8/8/8/8/8/8/R3K3 w - - 0 1"]          # RIGHT_LEFT without the right
CHECKMATE, STALEMATE = "7k/6Q1/6K1/8/8/8/8/8 b - - 0 1", "7k/5Q2/6K1/8/8/8/8/8 b - - 0 1"


def _oracle_lines(root):
    kids = list(root.children.values())
    lines = []
    for i in sorted(range(len(kids)), key=lambda i: (-kids[i].n, i))[:MULTIPV]:
        node = kids[i]
        pv = [node.move.uci()]
        while len(pv) < PV_LEN and node.expanded and node.children:
            best = None
            for c in node.children.values():
                if best is None or c.n > best.n:
                    best = c
            if best.n == 0:
                break
            pv.append(best.move.uci())
            node = best
        lines.append({"move": kids[i].move.uci(), "policy_index": kids[i].move_idx, "visits": kids[i].n, "prior": kids[i].prior,
                      "q": kids[i].q, "pv": pv})
    return lines


@pytest.mark.gpu
def test_analysis_engine_answers_table_roots_and_probes_the_rest(tb3):
    from matrix0_amd import analysis
    positions = TABLE_ROOTS[:3] + ROOTS[:2] + [CHECKMATE] + TABLE_ROOTS[3:] + ROOTS[2:] + [STALEMATE]
    ids = list(range(400, 400 + len(positions)))
    cfg = {"seed": 1234, "mcts": dict(MCTS, inference_batch_size=8), "selfplay": {"num_simulations": SIMS}}

    def run(slots, order):
        an = analysis.AnalyzerExt(FakeNet(seed=3, sharp=8.0).infer_np, cfg, slots=slots, multipv=MULTIPV, pv_len=PV_LEN,
                                  tablebase=tb3, tb_men=3)
        out = an.analyse([positions[i] for i in order], SIMS, ids=[ids[i] for i in order])
        leaves = an.engine.tb_leaves()
        an.close()
        return {r["id"]: r for r in out}, leaves

    got, leaves = run(3, list(range(len(positions))))
    for i, fen in enumerate(positions):
        g = got[ids[i]]
        if fen in TABLE_ROOTS:
            want = tb3.root_lines(fen, MULTIPV, PV_LEN)
            assert g["status"] == "tablebase" and g["evals"] == 0 and g["root_n"] == 0, fen
            assert {k: v for k, v in g.items() if k not in ("id", "fen", "moves")} == {k: v for k, v in want.items() if k != "id"}, fen
            py = su.py_root_lines(fen, tu.ref_tables(), MULTIPV, PV_LEN)
            assert [(ln["move"], ln["dtm"], ln["pv"]) for ln in g["lines"]] == [(ln["move"], ln["dtm"], ln["pv"]) for ln in py["lines"]]
            assert (g["root_q"], g["dtm"]) == (py["root_q"], py["dtm"]), fen
        elif fen in (CHECKMATE, STALEMATE):
            assert (g["status"], g["lines"], g["evals"]) == ("checkmate" if fen == CHECKMATE else "stalemate", [], 0)
        else:
            o, rq = oracle_run(fen, ids[i], 8, True)
            want = _oracle_lines(o._last_root)
            assert g["status"] == "ok" and "dtm" not in g and g["root_n"] == o._last_root.n and g["evals"] == o.evals, fen
            for key in ("move", "policy_index", "visits", "pv"):
                assert [ln[key] for ln in g["lines"]] == [ln[key] for ln in want], (fen, key)
            np.testing.assert_allclose([ln["prior"] for ln in g["lines"]], [ln["prior"] for ln in want], rtol=0, atol=1e-6)
            np.testing.assert_allclose([ln["q"] for ln in g["lines"]], [ln["q"] for ln in want], rtol=0, atol=1e-9)
            assert abs(g["root_q"] - rq) <= 1e-9, fen
    assert leaves == sum(oracle_run(fen, ids[i], 8, True)[0].tb_leaves for i, fen in enumerate(positions) if fen in ROOTS)
    # another order, another number of slots: the same results, bit for bit
    other, leaves2 = run(5, list(range(len(positions)))[::-1])
    assert sorted(other) == sorted(got) and leaves2 == leaves
    for k in got:
        assert other[k] == got[k], k
