"""Reading games back in, the parts that need no GPU: the token parser and the matching rule of csrc/san_match.h (compiled for the
host by tests/host_shim/replay_shim.cpp, with a scalar replay over gen_legal) against engine.san_legal and the oracle on the reference's own 125
evaluation games and on hand-made positions; the PGN reader; and import_pgn's filters, result handling and shard layout over a
fake replay_games that returns the shim's answers."""
import bz2
import os
import subprocess
import sys

import numpy as np
import pytest

from matrix0_amd import arena
from matrix0_amd import engine as eng
from matrix0_amd import game_import as gi
from oracle import chess_py as ch
from tests import replay_util as ru
from tests.replay_util import BISHOP, KING, KIND_EXACT, KIND_LONG, KIND_SAN, KIND_SHORT, KNIGHT, PAWN, QUEEN, ROOK, square

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# token -> (kind, piece type, from-file, from-rank, destination, promotion); -1 = not given
PATTERNS = {
    "e4": (KIND_SAN, PAWN, 4, -1, square("e4"), 0),
    "exd5": (KIND_SAN, PAWN, 4, -1, square("d5"), 0),
    "Nf3": (KIND_SAN, KNIGHT, -1, -1, square("f3"), 0),
    "Nbd7": (KIND_SAN, KNIGHT, 1, -1, square("d7"), 0),
    "R1e1": (KIND_SAN, ROOK, -1, 0, square("e1"), 0),
    "Qh4xe1": (KIND_SAN, QUEEN, 7, 3, square("e1"), 0),
    "e8=Q": (KIND_SAN, PAWN, 4, -1, square("e8"), 4),
    "e8Q": (KIND_SAN, PAWN, 4, -1, square("e8"), 4),
    "dxe8=N+": (KIND_SAN, PAWN, 3, -1, square("e8"), 1),
    "Kxe2#": (KIND_SAN, KING, -1, -1, square("e2"), 0),
    "e4!?": (KIND_SAN, PAWN, 4, -1, square("e4"), 0),
    "Bb5-c4": (KIND_SAN, BISHOP, 1, 4, square("c4"), 0),
    "a1=R": (KIND_SAN, PAWN, 0, -1, square("a1"), 3),
}
CASTLES = {"O-O": KIND_SHORT, "0-0-0+": KIND_LONG, "0-0": KIND_SHORT, "O-O-O": KIND_LONG, "O-O#": KIND_SHORT, "O-O-O!": KIND_LONG}
REJECTED = ["--", "Z0", "e9", "Xe4", "", "i4", "e", "4", "Ne", "=Q", "e8=K", "O-O-O-O", "0000", "e4e", "+", "Nf3++"]


def test_pattern_table():
    for tok, want in PATTERNS.items():
        rc, pat = ru.shim_pattern(tok)
        f = ru.pattern_fields(pat)
        assert rc == 0 and f["valid"] == 1, tok
        assert (f["kind"], f["type"], f["from_file"], f["from_rank"], f["to"], f["promo"]) == want, (tok, f)
    for tok, kind in CASTLES.items():
        rc, pat = ru.shim_pattern(tok)
        assert rc == 0 and ru.pattern_fields(pat)["kind"] == kind and ru.pattern_fields(pat)["valid"] == 1, tok
    for tok in REJECTED:
        assert ru.shim_pattern(tok) == (-1, 0), tok


def test_exact_patterns_and_the_library_agree_with_the_shim():
    # "b1c3" is a well-formed SAN pawn token and a UCI move: the caller names the kind
    f = ru.pattern_fields(ru.shim_pattern("b1c3", "uci")[1])
    assert (f["kind"], f["from_file"], f["from_rank"], f["to"], f["promo"]) == (KIND_EXACT, 1, 0, square("c3"), 0)
    f = ru.pattern_fields(ru.shim_pattern("b1c3", "san")[1])
    assert (f["kind"], f["type"], f["from_file"], f["from_rank"], f["to"]) == (KIND_SAN, PAWN, 1, 0, square("c3"))
    assert ru.shim_pattern("e7e8q", "uci")[1] == ru.shim_pattern(ru.raw_move("e7e8q"))[1]
    assert ru.pattern_fields(ru.shim_pattern("e7e8q", "uci")[1])["promo"] == 4
    for bad in ("0000", "e2e9", "e2", "e7e8k", "e2e4qq"):
        assert ru.shim_pattern(bad, "uci") == (-1, 0), bad
    assert ru.shim_pattern(0x8000) == (-1, 0) and ru.shim_pattern(5 << 12) == (-1, 0)
    # the library's host entry points are the same functions
    for tok in list(PATTERNS) + list(CASTLES) + REJECTED:
        assert gi.move_pattern(tok) == ru.shim_pattern(tok)[1], tok
    for u in ("b1c3", "e7e8q", "0000", "e2"):
        assert gi.move_pattern(u, "uci") == ru.shim_pattern(u, "uci")[1], u
    assert gi.move_pattern(ru.raw_move("g1f3")) == ru.shim_pattern(ru.raw_move("g1f3"))[1]
    assert gi.move_pattern(np.uint16(ru.raw_move("g1f3"))) == gi.move_pattern("g1f3", "uci")


def test_fixture_games_resolve_on_the_shim():
    """Every token of the 125 games resolves to exactly one move: the one whose SAN engine.san_legal writes with the same string,
    with the oracle's index, legal count, side to move and planes for the position it is played in."""
    games = ru.fixture_games()
    assert len(games) == 125
    n_tokens = promos = castles = mates = longest = 0
    for toks, _ in games:
        r = ru.shim_replay(None, toks, planes=True)
        assert r["status"] == "ok" and r["plies"] == len(toks)
        b = ch.Board()
        for k, tok in enumerate(toks):
            hits = [u for u, s in eng.san_legal(b.fen()) if s == tok]
            assert len(hits) == 1
            assert eng.move_to_uci(int(r["moves"][k])) == hits[0], (tok, b.fen())
            m = ch.Move.from_uci(hits[0])
            assert r["policy_idx"][k] == ch.move_to_index(b, m)
            assert r["nlegal"][k] == len(list(b.legal_moves)) and r["turn"][k] == int(b.turn)
            assert np.array_equal(r["planes"][k], ch.encode_board(b))
            promos += "=" in tok
            castles += tok.startswith("O-O")
            b.push(m)
        assert r["end"] == {"checkmate": b.is_checkmate(), "stalemate": b.is_stalemate(),
                            "insufficient": b.is_insufficient_material(), "white_to_move": bool(b.turn)}
        mates += r["end"]["checkmate"]
        n_tokens += len(toks)
        longest = max(longest, len(toks))
    assert (n_tokens, longest, promos, castles, mates) == (7875, 240, 39, 17, 96)


def test_fixture_games_as_uci_and_raw_moves_give_the_same_replay():
    for toks, _ in ru.fixture_games()[:10]:
        san = ru.shim_replay(None, toks)
        ucis = [eng.move_to_uci(int(m)) for m in san["moves"]]
        for other in (ru.shim_replay(None, ucis, "uci"), ru.shim_replay(None, [int(m) for m in san["moves"]])):
            assert other["status"] == "ok" and other["end"] == san["end"]
            for k in ("moves", "policy_idx", "nlegal", "turn"):
                assert np.array_equal(other[k], san[k])


@pytest.mark.parametrize("name", sorted(ru.HAND_CASES))
def test_hand_made_positions(name):
    fen, toks, max_plies, status, plies, moves = ru.hand_case(name)
    r = ru.shim_replay(fen, toks, max_plies=max_plies, planes=True)
    assert (r["status"], r["plies"]) == (status, plies)
    if moves is not None:
        assert [eng.move_to_uci(int(m)) for m in r["moves"][:plies]] == moves
    b = ch.Board(fen) if fen else ch.Board()
    for k in range(plies):                                   # the prefix is the oracle's game
        m = ch.Move.from_uci(eng.move_to_uci(int(r["moves"][k])))
        assert b.is_legal(m) and np.array_equal(r["planes"][k], ch.encode_board(b)) and r["turn"][k] == int(b.turn)
        b.push(m)
    for k in ("moves", "policy_idx", "nlegal", "turn", "planes"):
        assert not r[k][plies:].any()                        # rows after the stop stay zero


def test_en_passant_takes_the_pawn_off_the_board():
    fen, toks, *_ = ru.hand_case("en_passant")
    r = ru.shim_replay(fen, toks, planes=True)
    assert r["planes"][0][6, 3, 5] == 1.0 and r["planes"][1][6, 3, 5] == 0.0     # Black's f5 pawn: plane 6, row 8-5, file f


PGN_TEXT = """%escape line
[Event "first"]
[White "a \\"quoted\\" name"]
[Result "1-0"]

1.e4 {a comment with ) and 1. d4 in it} e5 $1 2. Nf3 (2. f4 exf4 (2... d5 $2) 3. Nf3) 2...Nc6 ; rest of the line 3. Bb5
3. Bb5!? a6 !? 4.Ba4 Nf6 1-0
[Event "second"]
[Result "0-1"]
[FEN "rnbqkbnr/pppppppp/8/8/4P3/8/PPPP1PPP/RNBQKBNR b KQkq e3 0 1"]

1... c5 2. Nf3 0-1

[Event "third"]
[Result "1/2-1/2"]

1. d4 d5 1/2-1/2 2. c4

[Event "fourth"]
[Result "*"]

1. c4 *
"""


def test_read_pgn(tmp_path):
    games = list(gi.read_pgn(PGN_TEXT))
    assert [h["Event"] for h, _ in games] == ["first", "second", "third", "fourth"]
    assert games[0][0]["White"] == 'a \\"quoted\\" name' and games[0][0]["Result"] == "1-0"
    assert games[0][1] == ["e4", "e5", "Nf3", "Nc6", "Bb5!?", "a6", "Ba4", "Nf6"]
    assert games[1][1] == ["c5", "Nf3"] and games[1][0]["FEN"].split()[1] == "b"
    assert games[2][1] == ["d4", "d5"] and games[3][1] == ["c4"]
    # the tokens replay: annotations are the parser's business, the FEN header is the start position
    for h, toks in games:
        r = ru.shim_replay(h.get("FEN"), toks)
        assert r["status"] == "ok" and r["plies"] == len(toks)
    plain, packed = tmp_path / "g.pgn", tmp_path / "g.pgn.bz2"
    plain.write_text(PGN_TEXT)
    packed.write_bytes(bz2.compress(PGN_TEXT.encode()))
    assert list(gi.read_pgn(str(plain))) == games and list(gi.read_pgn(packed)) == games


def test_save_pgn_output_reads_back(tmp_path):
    for i, (toks, result) in enumerate(ru.fixture_games()[:3]):
        raw = ru.shim_replay(None, toks)["moves"]
        path = arena.save_pgn(raw, result, {"Event": "fixture"}, str(tmp_path), i)
        (h, back), = gi.read_pgn(path)
        assert back == toks and h["Result"] == result and "FEN" not in h
        start = eng.fen_after(ch.START_FEN, [eng.move_to_uci(int(raw[0]))])      # the game without its first move
        path = arena.save_pgn(raw[1:], result, {"Event": "fixture"}, str(tmp_path), 10 + i, start_fen=start)
        (h, back), = gi.read_pgn(path)
        assert back == toks[1:] and h["FEN"] == start
        assert ru.shim_replay(h["FEN"], back)["plies"] == len(toks) - 1


def _pgn(games):
    out = []
    for headers, toks in games:
        out += [f'[{k} "{v}"]' for k, v in headers.items()] + ["", " ".join(toks + [headers.get("Result", "*")]), ""]
    return "\n".join(out)


MATE = ["f3", "e5", "g4", "Qh4#"]                            # Black mates
OPEN = ["e4", "e5", "Nf3"]


@pytest.fixture()
def fake_device(monkeypatch):
    monkeypatch.setattr(gi, "replay_games", ru.fake_replay_games)


def _load(out_dir):
    files = sorted(os.listdir(out_dir))
    return files, [np.load(os.path.join(out_dir, f)) for f in files]


def test_import_filters_and_summary(fake_device, tmp_path):
    good = {"Result": "0-1", "Termination": "Normal", "Site": "https://lichess.org/x", "WhiteElo": "2100", "BlackElo": "2200"}
    games = [
        (good, MATE),
        (dict(good, WhiteElo="1900"), OPEN),
        (dict(good, Termination="Time forfeit"), OPEN),
        (dict(good, Site="FICSGames 123"), OPEN),
        (dict(good, BlackElo="?"), OPEN),
        (dict(good, Result="*"), OPEN),
        ({"Result": "1-0"}, OPEN),                           # no Elo, no Termination
        (dict(good, Result="1/2-1/2"), []),                  # no moves
    ]
    text = _pgn(games)
    s = gi.import_pgn(text, str(tmp_path / "all"))
    # defaults: only the non-integer Elo, the unknown result and the empty game go
    assert s == {"games_read": 8, "games_kept": 5, "games_filtered": 3, "games_truncated": 0, "games_dropped": 0, "samples": 16,
                 "shards": 1, "result_mismatches": 0}
    s = gi.import_pgn(text, str(tmp_path / "lichess"), lichess=True)
    assert (s["games_kept"], s["games_filtered"], s["samples"]) == (1, 7, 4)
    s = gi.import_pgn(text, str(tmp_path / "elo"), min_elo=2000)
    assert (s["games_kept"], s["games_filtered"]) == (3, 5)
    s = gi.import_pgn(text, str(tmp_path / "term"), require_normal_termination=True)
    assert (s["games_kept"], s["games_filtered"]) == (3, 5)
    s = gi.import_pgn(text, str(tmp_path / "site"), skip_sites=("FICS",))
    assert (s["games_kept"], s["games_filtered"]) == (4, 4)
    s = gi.import_pgn(text, str(tmp_path / "cap"), max_games=2)
    assert (s["games_kept"], s["samples"]) == (2, 7)
    with pytest.raises(ValueError):
        gi.import_pgn(text, str(tmp_path / "bad"), on_error="ignore")
    with pytest.raises(ValueError):
        gi.import_pgn(text, str(tmp_path / "bad"), result_source="engine")


def test_import_samples_errors_and_result_source(fake_device, tmp_path):
    games = [
        ({"Result": "1-0"}, MATE),                           # the header names the wrong winner
        ({"Result": "1-0"}, ["e4", "e5", "Ke3", "Nc6"]),     # stops at ply 2
        ({"Result": "1/2-1/2"}, ["Ke2"]),                    # stops at ply 0
        ({"Result": "*"}, MATE),                             # only the board knows
        ({"Result": "0-1", "FEN": "rnbqkbnr/pppppppp/8/8/4P3/8/PPPP1PPP/RNBQKBNR b KQkq e3 0 1"}, ["e5", "Nf3"]),
    ]
    text = _pgn(games)
    s = gi.import_pgn(text, str(tmp_path / "h"), shard_size=3, legal_mask=True, ssl_tasks=("piece", "control"))
    assert s == {"games_read": 5, "games_kept": 3, "games_filtered": 1, "games_truncated": 1, "games_dropped": 1, "samples": 8,
                 "shards": 3, "result_mismatches": 1}
    files, shards = _load(tmp_path / "h")
    assert files == ["import_000000.npz", "import_000001.npz", "import_000002.npz"]
    assert [len(d["z"]) for d in shards] == [3, 3, 2]
    for d in shards:
        n = len(d["z"])
        assert sorted(d.files) == ["legal_mask", "pi", "s", "ssl_control", "ssl_piece", "z"]
        assert (d["s"].dtype, d["s"].shape) == (np.float32, (n, 19, 8, 8)) and (d["pi"].dtype, d["pi"].shape) == (np.float32, (n, 4672))
        assert (d["z"].dtype, d["z"].shape) == (np.float32, (n,)) and (d["legal_mask"].dtype, d["legal_mask"].shape) == (np.uint8, (n, 4672))
        assert d["ssl_piece"].shape == (n, 13, 8, 8) and d["ssl_control"].shape == (n, 8, 8)
        assert np.array_equal(d["pi"], d["legal_mask"].astype(np.float32))      # the fake mask holds the played move only
    z = np.concatenate([d["z"] for d in shards])
    assert z.tolist() == [1, -1, 1, -1] + [1, -1] + [1, -1]  # header 1-0 from the mover's side; 0-1 with Black to move first
    s0 = np.concatenate([d["s"] for d in shards])
    assert np.array_equal(s0[0], ch.encode_board(ch.Board())) and np.array_equal(s0[6], ch.encode_board(ch.Board(games[4][0]["FEN"])))
    pi = np.concatenate([d["pi"] for d in shards])
    assert pi[0].argmax() == ch.move_to_index(ch.Board(), ch.Move.from_uci("f2f3")) and pi.sum(axis=1).tolist() == [1.0] * 8

    s = gi.import_pgn(text, str(tmp_path / "b"), result_source="board", on_error="drop", legal_mask=False, prefix="x")
    assert s == {"games_read": 5, "games_kept": 3, "games_filtered": 0, "games_truncated": 0, "games_dropped": 2, "samples": 10,
                 "shards": 1, "result_mismatches": 1}
    files, (d,) = _load(tmp_path / "b")
    assert files == ["x_000000.npz"] and sorted(d.files) == ["pi", "s", "z"]
    assert d["z"].tolist() == [-1, 1, -1, 1] * 2 + [1, -1]   # Black mated: White's samples carry -1
    assert not [f for f in os.listdir(tmp_path / "b") if f.endswith(".tmp")]


def test_cli_help():
    r = subprocess.run([sys.executable, "-m", "matrix0_amd.game_import", "--help"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and "--result-source" in r.stdout and "--lichess" in r.stdout
