"""Opening book for evaluation matches, paired by colour (`eval.openings_pgn` / play_match(openings=...),
m0_selfplay_cfg.arena_paired_openings): games 2k and 2k+1 start from the same book position, drawn from a counter stream of
pair k's own, so the pairing depends on neither the slot nor the order in which the games start."""
import os

import pytest

from oracle import chess_py as ch
from oracle import mcts_ref as ref
from oracle import net_ref

pytestmark = pytest.mark.gpu

BOOK_PGN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "main_eval_book.pgn")
NET = dict(planes=19, channels=32, blocks=2, attention_heads=2, policy_size=4672, norm="group", activation="silu",
           preact=True, policy_factor_rank=0, self_supervised=False)
CFG = {"seed": 7,
       "mcts": {"cpuct": 2.5, "cpuct_start": 3.0, "cpuct_end": 2.0, "cpuct_plies": 40, "dirichlet_plies": 30,
                "dirichlet_frac": 0.25, "selection_jitter": 0.0, "fpu_reduction": 0.1, "draw_penalty": -0.05,
                "legal_softmax": True, "inference_batch_size": 8, "playout_random_frac": 0.0},
       "selfplay": {"selection_jitter": 0.0},
       "eval": {"max_moves": 40},
       "draw": {"min_plies": 30, "window": 8, "min_unique": 4, "halfmove_cap": 100}}
SEED = 3                  # draws four different book positions for the four pairs (checked below, on the CPU side of the test)
PURPOSE_PAIR_OPENING = 5  # csrc/host_rules.h


def _backends():
    from matrix0_amd.backend import M0Backend
    return (M0Backend.from_state_dict(NET, net_ref.random_state_dict(NET, seed=1)),
            M0Backend.from_state_dict(NET, net_ref.random_state_dict(NET, seed=2)))


def _pair_draw(seed, k, n):
    return min(int(ref.Stream(ref.derive_seed(seed, k, PURPOSE_PAIR_OPENING)).next() * n), n - 1)


def test_paired_openings_from_the_pgn_book(tmp_path):
    from matrix0_amd import arena, pgn_book
    book = pgn_book.load_opening_book(BOOK_PGN)
    assert len(set(book)) >= 2
    want = [_pair_draw(SEED, k, len(book)) for k in range(4)]
    assert len({book[i] for i in want}) >= 2, "pick a seed that draws at least two different positions"
    a, b = _backends()
    cfg = dict(CFG, eval=dict(CFG["eval"], openings_pgn=BOOK_PGN))
    by_conc = {}
    for conc in (2, 8):
        arena.play_match(a, b, 8, cfg, seed=SEED, num_sims=16, temp=1.0, temp_plies=4, max_moves_override=10,
                         concurrent_games=conc, leaves_per_step=8, pgn_out=str(tmp_path / f"pgn{conc}"))
        recs = {r["game_index"]: r for r in arena.last_match_stats["records"]}
        assert sorted(recs) == list(range(8))
        by_conc[conc] = recs
        for k in range(4):
            assert recs[2 * k]["start_fen"] == recs[2 * k + 1]["start_fen"] == book[want[k]], k
        assert len({r["start_fen"] for r in recs.values()}) >= 2
        for i, r in recs.items():
            assert r["start_fen"] in book
            board = ch.Board(r["start_fen"])
            assert 1 <= len(r["played"]) <= 10 and r["moves"] == len(r["played"])     # max_moves counts from the book position
            for u in r["played"]:
                m = ch.Move.from_uci(u)
                assert m in board.legal_moves, (i, u)
                board.push(m)
            txt = (tmp_path / f"pgn{conc}" / f"game_{i:04d}.pgn").read_text()
            assert '[SetUp "1"]' in txt and f'[FEN "{r["start_fen"]}"]' in txt
            first = txt.split("\n\n", 1)[1].split()[0]
            fullmove = r["start_fen"].split()[5]
            assert first == (f"{fullmove}." if r["start_fen"].split()[1] == "w" else f"{fullmove}...")
    # the same seed pairs the games the same way whatever the number of slots and the order in which the games start
    assert {i: r["start_fen"] for i, r in by_conc[2].items()} == {i: r["start_fen"] for i, r in by_conc[8].items()}
    a.close(); b.close()


def test_without_a_book_pairing_changes_nothing():
    from matrix0_amd import arena, engine as eng
    a, b = _backends()

    def match(paired):
        c = arena.arena_cfg_from_dict(CFG, games=3, num_sims=16, max_moves=12, temp=1.0, temp_plies=10, concurrent_games=3,
                                      leaves_per_step=8, seed=5)
        c.arena_paired_openings = paired
        e = eng.ArenaEngine(a, b, c)
        e.set_openings([])
        recs = {}
        while e.running():
            e.step(8)
            while (r := e.poll()) is not None:
                assert "start_fen" not in r
                recs[r["game_index"]] = r["played"]
        e.close()
        return recs

    g0, g1 = match(0), match(1)
    assert sorted(g0) == [0, 1, 2] and g0 == g1
    arena.play_match(a, b, 3, CFG, seed=5, num_sims=16, temp=1.0, temp_plies=10, max_moves_override=12, concurrent_games=3,
                     leaves_per_step=8)
    a.close(); b.close()
    assert {r["game_index"]: r["played"] for r in arena.last_match_stats["records"]} == g0
    assert all("start_fen" not in r for r in arena.last_match_stats["records"])
