"""Host side of the match additions (no GPU): the config keys of the per-side evaluation cache, the opening book's way from
`eval.openings_pgn` / `openings=` to the engine call, and PGN output of games that start from a book position."""
import os

import numpy as np
import pytest

from matrix0_amd import arena
from matrix0_amd import engine as eng

BOOK_PGN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "main_eval_book.pgn")
KW = dict(games=4, num_sims=16, max_moves=20, temp=0.0, temp_plies=0, concurrent_games=2, leaves_per_step=8, seed=1)


def _raw(ucis):
    def sq(s):
        return "abcdefgh".index(s[0]) + 8 * (int(s[1]) - 1)
    return np.array([sq(u[:2]) | sq(u[2:4]) << 6 | (" nbrq".index(u[4]) if len(u) > 4 else 0) << 12 for u in ucis], np.uint16)


def test_arena_cfg_maps_the_cache_keys_and_leaves_eval_cache_off():
    c = arena.arena_cfg_from_dict({}, **KW)
    assert (c.arena_eval_cache, c.eval_cache_entries, c.eval_cache, c.arena_paired_openings) == (0, 0, 0, 0)
    c = arena.arena_cfg_from_dict({"engine": {"arena_eval_cache": True, "eval_cache_entries": 4096, "eval_cache": True}}, **KW)
    assert (c.arena_eval_cache, c.eval_cache_entries, c.eval_cache) == (1, 4096, 0)
    # appended behind tail_split: every earlier field keeps its offset
    names = [n for n, _ in eng.SelfplayCfg._fields_]
    assert names[-3:] == ["tail_split", "arena_eval_cache", "arena_paired_openings"]
    assert [n for n, _ in eng.GameRecord._fields_][-2:] == ["owner", "start_fen"]


class _FakeArenaEngine:
    """Stands in for eng.ArenaEngine: records what play_match hands over and plays no game."""
    made = []

    def __init__(self, a, b, cfg):
        self.cfg, self.book, self.stepped_before_book = cfg, None, False
        self.steps = 0
        _FakeArenaEngine.made.append(self)

    def set_openings(self, fens):
        self.stepped_before_book = self.steps > 0
        self.book = list(fens)

    def running(self):
        return self.steps == 0

    def step(self, n):
        self.steps += 1

    def poll(self):
        return None

    def stats(self):
        return {"evals": 0, "evals_cached": 0, "plies": 0}

    def close(self):
        pass


@pytest.fixture
def fake_engine(monkeypatch):
    _FakeArenaEngine.made = []
    monkeypatch.setattr(eng, "ArenaEngine", _FakeArenaEngine)
    return _FakeArenaEngine.made


def test_play_match_hands_the_book_to_the_engine(fake_engine):
    from matrix0_amd import pgn_book
    book = pgn_book.load_opening_book(BOOK_PGN)
    assert len(book) >= 2
    # eval.openings_pgn
    arena.play_match(None, None, 4, {"eval": {"openings_pgn": BOOK_PGN}}, num_sims=8)
    e = fake_engine[-1]
    assert e.book == book and not e.stepped_before_book and e.cfg.arena_paired_openings == 1 and e.steps == 1
    # an explicit list wins over the key
    fens = [book[1], book[0]]
    arena.play_match(None, None, 4, {"eval": {"openings_pgn": BOOK_PGN}}, num_sims=8, openings=fens)
    assert fake_engine[-1].book == fens and fake_engine[-1].cfg.arena_paired_openings == 1
    # neither: the initial position, as before
    arena.play_match(None, None, 4, {}, num_sims=8)
    assert fake_engine[-1].book is None and fake_engine[-1].cfg.arena_paired_openings == 0
    arena.play_match(None, None, 4, {"eval": {"openings_pgn": BOOK_PGN}}, num_sims=8, openings=[])
    assert fake_engine[-1].book is None and fake_engine[-1].cfg.arena_paired_openings == 0
    assert arena.last_match_stats["evals_cached"] == 0.0
    # a book file without positions is reported, and the match starts from the initial position
    with pytest.warns(UserWarning, match="openings_pgn"):
        arena.play_match(None, None, 4, {"eval": {"openings_pgn": BOOK_PGN + ".missing"}}, num_sims=8)
    assert fake_engine[-1].book is None


def test_play_match_passes_the_cache_switch(fake_engine):
    arena.play_match(None, None, 2, {"engine": {"arena_eval_cache": True, "eval_cache_entries": 8192}}, num_sims=8)
    c = fake_engine[-1].cfg
    assert (c.arena_eval_cache, c.eval_cache_entries, c.eval_cache) == (1, 8192, 0)
    arena.play_match(None, None, 2, {}, num_sims=8)
    assert fake_engine[-1].cfg.arena_eval_cache == 0


BLACK_FIRST = "rnbqkbnr/pppp1ppp/8/4p3/4P3/5N2/PPPP1PPP/RNBQKB1R b KQkq - 1 12"
WHITE_FIRST = "r1bqkbnr/pppp1ppp/2n5/4p3/4P3/5N2/PPPP1PPP/RNBQKB1R w KQkq - 2 3"


def test_movetext_from_a_fen_follows_its_move_number():
    assert eng.san_game(_raw(["g8f6", "b1c3", "b8c6", "f1b5"]), BLACK_FIRST) == "12... Nf6 13. Nc3 Nc6 14. Bb5"
    assert eng.san_game(_raw(["g8f6"]), BLACK_FIRST) == "12... Nf6"
    assert eng.san_game(_raw(["f1b5", "a7a6", "b5c6", "d7c6"]), WHITE_FIRST) == "3. Bb5 a6 4. Bxc6 dxc6"
    assert eng.san_game(_raw([]), BLACK_FIRST) == ""
    # the start position through both entry points
    start = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1"
    mv = _raw(["e2e4", "e7e5", "g1f3"])
    assert eng.san_game(mv) == eng.san_game(mv, start) == "1. e4 e5 2. Nf3"
    with pytest.raises(ValueError):
        eng.san_game(_raw(["e2e4"]), BLACK_FIRST)              # not legal there
    with pytest.raises(ValueError):
        eng.san_game(mv, "not a fen")


def test_setup_and_fen_tags_only_for_book_games(tmp_path):
    hdr = {"Event": "Matrix0 arena", "Round": 1, "White": "A", "Black": "B", "Date": "2025.01.01"}
    mv = _raw(["e2e4", "e7e5", "g1f3"])
    plain = open(arena.save_pgn(mv, "1/2-1/2", hdr, str(tmp_path / "plain"), 0)).read()
    assert plain == ('[Event "Matrix0 arena"]\n[Site "?"]\n[Date "2025.01.01"]\n[Round "1"]\n[White "A"]\n[Black "B"]\n'
                     '[Result "1/2-1/2"]\n\n1. e4 e5 2. Nf3 1/2-1/2\n')
    assert "SetUp" not in plain and "FEN" not in plain
    assert open(arena.save_pgn(mv, "1/2-1/2", hdr, str(tmp_path / "none"), 0, start_fen=None)).read() == plain
    book = open(arena.save_pgn(_raw(["g8f6", "b1c3"]), "0-1", hdr, str(tmp_path / "book"), 3, start_fen=BLACK_FIRST)).read()
    assert book == ('[Event "Matrix0 arena"]\n[Site "?"]\n[Date "2025.01.01"]\n[Round "1"]\n[White "A"]\n[Black "B"]\n'
                    f'[Result "0-1"]\n[SetUp "1"]\n[FEN "{BLACK_FIRST}"]\n\n12... Nf6 13. Nc3 0-1\n')
