"""Endgame tablebases on the GPU: the built tables against the independent generator (byte for byte for KK and the 3-man
tables, by certificate for 4-man tables), probing, and the self-play game loop ending games on a hit."""
import ctypes as C

import numpy as np
import pytest

from tests import tb_util as tu
from tests.hash_net import HashNet

pytestmark = pytest.mark.gpu

START = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1"


@pytest.fixture(scope="module")
def tb3():
    from matrix0_amd.tablebase import Tablebase
    tb = Tablebase.build(3, 0)
    yield tb
    tb.close()


def test_three_man_build_equals_the_reference_generator(tb3):
    ref = tu.ref_tables()
    info = {i["sig"]: i for i in tb3.info()}
    # build order: by men, then pawns, then name -- KK first, KPK (which promotes into the others) last
    assert tb3.max_men == 3 and sorted(info) == sorted(tu.THREE_MAN) and list(info)[0] == "KK" and list(info)[-1] == "KPK"
    for s in tu.THREE_MAN:
        got = tb3.table(s)
        print(f"{s}: largest d {info[s]['max_d']}, {info[s]['sweeps']} sweeps, {info[s]['build_ms']:.1f} ms")
        assert np.array_equal(got, ref[s]), f"{s}: {int((got != ref[s]).sum())} entries differ"
    assert {s: info[s]["max_d"] for s in tu.THREE_MAN} == {"KK": -1, "KQK": 20, "KRK": 32, "KBK": -1, "KNK": -1, "KPK": 56}


def _certified(sig, expect_tables, tmp_path, twice):
    """Build `sig` with its dependencies (twice: byte-identical), then the reference's certificate check: 200 000 entries drawn
    with a fixed seed plus every entry with d <= 2, zero violations, nothing skipped."""
    from matrix0_amd.tablebase import Tablebase
    tb = Tablebase.build_signatures([sig], 0)
    names = [i["sig"] for i in tb.info()]
    assert set(names) == set(expect_tables) and names[-1] == sig
    tables = {s: tb.table(s) for s in names}
    for i in tb.info():
        print(f"{i['sig']}: largest d {i['max_d']}, {i['sweeps']} sweeps, {i['build_ms']:.1f} ms")
        assert i["max_d"] < 254
    tb.close()
    if twice:
        tb2 = Tablebase.build_signatures([sig], 0)
        for s in names:
            assert np.array_equal(tb2.table(s), tables[s]), f"two builds of {s} differ"
        tb2.close()
    rc, res, out = tu.certificate(tables, sig, 20260, 200000, str(tmp_path))
    print(out)
    assert rc == 0 and res["violations"] == 0 and res["skipped"] == 0, out
    assert res["sampled"] == 200000 and res["checked"] == 200000 + res["low_d"] and res["low_d"] > 0


def test_kqkr_build_is_reproducible_and_certified(tmp_path):
    _certified("KQKR", ["KK", "KQK", "KRK", "KQKR"], tmp_path, twice=True)


def test_krpk_with_its_promotion_tables_is_certified(tmp_path):
    _certified("KRPK", ["KK", "KQK", "KRK", "KBK", "KNK", "KPK", "KQRK", "KRRK", "KRBK", "KRNK", "KRPK"], tmp_path, twice=False)


def test_probing(tb3):
    fens = ["4k3/8/8/8/8/8/8/4K2R w K - 0 1",          # a castling right left
            "4k3/8/8/8/8/8/8/4K2R w - - 0 1",
            "4k3/4p3/8/8/8/8/4P3/4K3 w - - 0 1",       # KPKP
            "4k3/8/8/8/8/8/PPP5/4K3 w - - 0 1",        # 5 men
            "8/8/8/3k4/8/8/1q6/7K w - - 0 1",          # Black is the greater side, White to move: lost
            "8/8/8/3k4/8/8/1q6/7K b - - 0 1",          # ... Black to move: won
            "8/8/8/8/8/6k1/6q1/7K w - - 0 1",          # White is checkmated
            "7k/6Q1/6K1/8/8/8/8/8 b - - 0 1"]          # Black is checkmated
    hit, wdl, dtm = tb3.probe(fens)
    assert hit.tolist() == [False, True, False, False, True, True, True, True]
    assert int(wdl[1]) == 1 and int(dtm[1]) % 2 == 1
    assert int(wdl[4]) == -1 and int(dtm[4]) % 2 == 0 and int(dtm[4]) > 0
    assert int(wdl[5]) == 1 and int(dtm[5]) % 2 == 1
    assert (int(wdl[6]), int(dtm[6])) == (-1, 0) and (int(wdl[7]), int(dtm[7])) == (-1, 0)
    # ... and against the flipped position's entry of the reference table
    ref = tu.ref_tables()["KQK"]
    l = tu.shim()
    code, idx = C.c_int(0), C.c_uint32(0)
    for k in (4, 5):
        assert l.tbs_locate(fens[k].encode(), C.byref(code), C.byref(idx)) == 1 and code.value == l.tbs_sig_code(b"KQK")
        assert (int(wdl[k]), int(dtm[k])) == tu.entry_wdl_dtm(int(ref[idx.value]))


MCTS = {"cpuct": 2.5, "dirichlet_plies": 30, "selection_jitter": 0.05, "fpu_reduction": 0.1, "draw_penalty": -0.05,
        "legal_softmax": True, "inference_batch_size": 4}
# Kings far apart: no first move mates or stalemates.  KQK / KRK: White moves, the probed position has Black to move.
# kqK: the same with Black as the greater side and to move, so the probed position has White to move and loses.  KPK: a rook
# pawn with the defending king in front of it, drawn whatever is played.  KBK is over before a move (insufficient material).
BOOK = {"KQK": "8/8/8/4k3/8/8/8/KQ6 w - - 0 1", "KRK": "8/8/8/4k3/8/8/8/KR6 w - - 0 1", "kqK": "8/8/8/4K3/8/8/8/kq6 b - - 0 1",
        "KPK": "8/8/8/8/8/k7/P7/K7 w - - 0 1", "KBK": "8/8/8/4k3/8/8/8/KB6 w - - 0 1"}


def _play(book, tb, games, max_game_len, seed=11):
    from matrix0_amd import engine as eng
    cfg = eng.selfplay_cfg_from_dict({"seed": seed, "mcts": MCTS,
                                      "selfplay": {"num_simulations": 8, "max_game_len": max_game_len, "opening_random_plies": 0}},
                                     concurrent_games=games, total_games=games)
    e = eng.SelfplayEngine(None, cfg)
    if book:
        e.set_openings(book)
    if tb is not None:
        e.set_tablebase(tb, 4)
    net = HashNet(seed=5, sharp=8.0)
    recs = []
    for _ in range(20000):
        if not e.running():
            break
        planes = e.ext_select()
        lg, v = net.infer_np(planes) if planes.shape[0] else (np.zeros((0, 4672), np.float32), np.zeros((0,), np.float32))
        e.ext_expand(lg, v)
        while True:
            r = e.poll()
            if r is None:
                break
            recs.append(r)
    assert not e.running()
    hits = e.tb_adjudications()
    assert int(e.stats()["games_finished"]) == games
    e.close()
    return sorted(recs, key=lambda r: r["game_index"]), hits


def test_game_loop_ends_games_on_a_tablebase_hit(tb3):
    from matrix0_amd import engine as eng
    book = [BOOK["KQK"], BOOK["KRK"], BOOK["kqK"], BOOK["KPK"]]
    games = 16
    with_tb, hits = _play(book, tb3, games, 8)
    without, hits0 = _play(book, None, games, 8)
    assert len(with_tb) == len(without) == games and hits0 == 0 and hits == games
    assert {r["start_fen"] for r in with_tb} == set(book), "the seed must draw every book position"
    for r, r0 in zip(with_tb, without):
        assert r["start_fen"] == r0["start_fen"] and not r["resigned"] and r["resigner"] is None
        assert r["moves"] == 1 and len(r["played"]) == 1 and r0["moves"] > 1
        assert r["played"][0] == r0["played"][0]                      # the same game up to the hit
        after = eng.fen_after(r["start_fen"], r["played"])
        hit, wdl, _ = tb3.probe([after])
        assert hit[0]
        stm_white = after.split()[1] == "w"
        assert stm_white == (r["start_fen"] == BOOK["kqK"])
        assert r["result"] == float(wdl[0]) * (1.0 if stm_white else -1.0) and r["draw"] == (wdl[0] == 0)
        # the one recorded ply belongs to the side that moved: its z is the result from that side
        assert np.array_equal(r["z"], np.array([r["result"] * (-1.0 if stm_white else 1.0)], np.float32))
        if r["start_fen"] == BOOK["KPK"]:
            assert r["result"] == 0.0 and r["draw"]
        if r["start_fen"] == BOOK["kqK"]:
            assert r["result"] in (-1.0, 0.0)                         # White to move and lost, unless the queen was hung
    assert any(r["result"] == 1.0 for r in with_tb) and any(r["result"] == -1.0 for r in with_tb)
    # KBK: the position is over before a move is played (insufficient material, as in the reference's loop), so there is no
    # ply, no probe and no record, with or without the tables
    for tb in (tb3, None):
        recs, hits = _play([BOOK["KBK"]], tb, 2, 8)
        assert recs == [] and hits == 0


def test_games_without_a_hit_are_bit_identical(tb3):
    a, hits = _play([], tb3, 4, 6)
    b, _ = _play([], None, 4, 6)
    assert hits == 0 and len(a) == len(b) == 4
    for x, y in zip(a, b):
        assert "start_fen" not in x and "start_fen" not in y
        for k in ("game_index", "moves", "resigned", "resigner", "draw", "result", "avg_policy_entropy", "avg_sims", "played"):
            assert x[k] == y[k], k
        for k in ("s", "pi", "z", "legal_mask", "search_values", "played_raw"):
            assert x[k].tobytes() == y[k].tobytes(), k


def test_set_tablebase_is_refused_by_match_and_analysis_engines(tb3):
    from matrix0_amd import _lib, engine as eng
    cfg = eng.selfplay_cfg_from_dict({"mcts": MCTS, "selfplay": {"num_simulations": 8}}, concurrent_games=2, total_games=2)
    for e in (eng.ArenaExtEngine(cfg), eng.AnalysisExtEngine(cfg)):
        with pytest.raises(RuntimeError, match="self-play engines only"):
            e.set_tablebase(tb3, 3)
        assert e._L.m0_selfplay_set_tablebase(e._h, tb3.handle, 3) == _lib.M0_ERR_STATE
        e.close()
    # a self-play engine takes it before the first step only
    e = eng.SelfplayEngine(None, cfg)
    e.set_tablebase(tb3, 3)
    e.set_tablebase(None)
    planes = e.ext_select()
    e.ext_expand(*HashNet(seed=5, sharp=8.0).infer_np(planes))
    assert e._L.m0_selfplay_set_tablebase(e._h, tb3.handle, 3) == _lib.M0_ERR_STATE
    e.close()
