"""The rules corpus of tests/rules_cases.py on the CPU: that it holds what it is there for (a census counted with the oracle), that
its move sequences are perft (the published counts), and that the host builds of the product's rules (csrc/chess_core.h through
tests/host_shim/chess_shim.cpp, csrc/san_match.h and the scalar replay through replay_shim.cpp) agree with the oracle on every
position and every sequence of it.  tests/test_rules_edges_gpu.py asks the same of the device kernels."""
import ctypes as C

import numpy as np
import pytest

from oracle import chess_py as ch
from tests import host_shim
from tests import replay_util as ru
from tests import rules_cases as rc


@pytest.fixture(scope="module")
def census():
    """Per position of the two-ply neighbourhood what the oracle says of it."""
    rows = []
    for fen in rc.neighbourhood(2):
        b = ch.Board(fen)
        lm = b.legal_moves
        pseudo = rc.pseudo_en_passant(b)
        legal_ep = [m for m in lm if rc.is_en_passant(b, m)]
        assert {(m.from_square, m.to_square) for m in legal_ep} <= set(pseudo), fen
        rows.append({"fen": fen, "n": len(lm), "check": len(rc.checkers(b)), "ep_legal": len(legal_ep),
                     "ep_illegal": len(pseudo) - len(legal_ep)})
    return rows


def _castles(b):
    return sorted(m.uci() for m in b.legal_moves
                  if b.piece_type_at(m.from_square) == ch.KING and abs((m.from_square & 7) - (m.to_square & 7)) == 2)


def _seventh_rank_pawns(b):
    return [s for s in b.pieces(ch.PAWN, b.turn) if (s >> 3) == (6 if b.turn else 1)]


def _only_king_moves(b):
    return all(b.piece_type_at(m.from_square) == ch.KING for m in b.legal_moves)


def _illegal_ep(b):
    return bool(rc.pseudo_en_passant(b)) and not any(rc.is_en_passant(b, m) for m in b.legal_moves)


def _pawn_checker(b):
    """The pawn that has just made its double step is the one checker."""
    return b.ep_square is not None and rc.checkers(b) == [b.ep_square + (-8 if b.turn else 8)]


def _double_check_in_one(b):
    for m in b.legal_moves:
        b.push(m)
        n = len(rc.checkers(b))
        b.pop()
        if n == 2:
            return True
    return False


def _pinned_promotion(b):
    """A pawn on its seventh rank, an empty square before it, no check, and yet no push."""
    step = 8 if b.turn else -8
    return not b.is_check() and any(not b.piece_code_at(s + step) and not b.is_legal(ch.Move(s, s + step, ch.QUEEN))
                                    for s in _seventh_rank_pawns(b))


# class -> what a root filed under it must show, by the oracle
CLASS_HOLDS = {
    "ep_legal": lambda b: sum(rc.is_en_passant(b, m) for m in b.legal_moves) == 1,
    "ep_illegal_rank": lambda b: _illegal_ep(b) and not b.is_check(),
    "ep_illegal_pinned_file": lambda b: _illegal_ep(b) and not b.is_check(),
    "ep_illegal_pinned_diagonal": lambda b: _illegal_ep(b) and not b.is_check(),
    "ep_illegal_shield_diagonal": lambda b: _illegal_ep(b) and not b.is_check(),
    "ep_removes_checker": lambda b: _pawn_checker(b) and any(rc.is_en_passant(b, m) for m in b.legal_moves),
    "ep_two_capturers": lambda b: sum(rc.is_en_passant(b, m) for m in b.legal_moves) == 2,
    "ep_no_capturer": lambda b: b.ep_square is not None and not rc.pseudo_en_passant(b),
    "ep_in_check": lambda b: b.is_check() and bool(rc.pseudo_en_passant(b)) and not _pawn_checker(b),
    "double_check": lambda b: len(rc.checkers(b)) == 2 and _only_king_moves(b) and len(b.piece_map()) > 4,
    "before_double_check": _double_check_in_one,
    "check_answers": lambda b: len(rc.checkers(b)) == 1 and not _only_king_moves(b),
    "check_all_pinned": lambda b: len(rc.checkers(b)) == 1 and _only_king_moves(b) and b.legal_moves and
    sum((c <= 6) == b.turn for c in b.piece_map().values()) >= 4,
    "promotion": lambda b: {m.promotion for m in b.legal_moves} >= {ch.KNIGHT, ch.BISHOP, ch.ROOK, ch.QUEEN},
    "promotion_pinned": _pinned_promotion,
    "wide": lambda b: len(b.legal_moves) > 128,
    "wave_edge": lambda b: len(b.legal_moves) in (63, 64, 65, 127, 128, 129),
    "terminal": lambda b: not b.legal_moves and (b.is_checkmate() or b.is_stalemate()),
    "perft": lambda b: True,
}


def test_every_root_shows_what_its_class_says():
    assert len(rc.ROOTS) >= 60
    for name, cls, fen in rc.ROOTS:
        b = ch.Board(fen)
        f = fen.split(" ")
        other = " ".join([f[0], "b" if f[1] == "w" else "w", f[2], "-", f[4], f[5]])
        assert not ch.Board(other).is_check(), name                       # a legal position: the side that has moved is not in check
        if name in rc.CASTLES_LEFT:
            assert f[2] in ("KQ", "kq") and _castles(b) == rc.CASTLES_LEFT[name], name
        else:
            assert CLASS_HOLDS[cls](b), name
    assert set(rc.CLASSES) == set(CLASS_HOLDS) | {c for _, c, _, _ in rc._CASTLING}
    for n, fen in rc.WAVE_EDGE.items():
        assert len(ch.Board(fen).legal_moves) == n
    for fen in (rc.WIDE_218, rc.WIDE_218_B):
        assert len(ch.Board(fen).legal_moves) == 218
    assert len(ch.Board(rc.WIDE_138).legal_moves) == len(ch.Board(rc.mirror(rc.WIDE_138)).legal_moves) == 138
    both = [ch.Board(f) for n, c, f in rc.ROOTS if c == "terminal"]
    assert any(b.is_checkmate() for b in both) and any(b.is_stalemate() for b in both)
    # push and both captures, for each colour
    for name in ("promotion_white_push_and_captures", "promotion_black_push_and_captures"):
        b = ch.Board(rc.ROOT_FEN[name])
        (pawn,) = _seventh_rank_pawns(b)
        files = sorted((m.to_square & 7) - (pawn & 7) for m in b.legal_moves if m.from_square == pawn)
        assert files == [-1] * 4 + [0] * 4 + [1] * 4


def test_census_of_the_neighbourhood(census):
    """Conditions on the corpus, not measurements of it: a root is added when a floor is not met."""
    nb = rc.neighbourhood(2)
    assert len(census) == len(nb) == len(set(nb)) and 7000 <= len(nb) <= 20000
    assert set(nb) >= {rc.fen_raw(ch.Board(f)) for _, _, f in rc.ROOTS}            # so every class is in it
    n = np.array([r["n"] for r in census])
    check = np.array([r["check"] for r in census])
    figures = {
        "positions": len(nb),
        "legal en passant": int(sum(r["ep_legal"] > 0 for r in census)),
        "illegal en passant": int(sum(r["ep_illegal"] > 0 for r in census)),
        "64 moves": int((n == 64).sum()), "65 moves": int((n == 65).sum()),
        "(64, 128]": int(((n > 64) & (n <= 128)).sum()), "(128, 192]": int(((n > 128) & (n <= 192)).sum()),
        "(192, 218]": int(((n > 192) & (n <= 218)).sum()),
        "in check": int((check > 0).sum()), "double check": int((check == 2).sum()), "no legal move": int((n == 0).sum()),
    }
    print("rules corpus census:", figures)
    assert figures["legal en passant"] >= 5 and figures["illegal en passant"] >= 3
    assert figures["64 moves"] >= 1 and figures["65 moves"] >= 1
    assert figures["(64, 128]"] >= 1 and figures["(128, 192]"] >= 1 and figures["(192, 218]"] >= 1
    assert figures["in check"] >= 50 and figures["double check"] >= 3 and figures["no legal move"] >= 20
    assert check.max() == 2 and n.max() == 218


@pytest.mark.parametrize("name,depth,count", [p for p in rc.PERFT_PATHS if p[2] is not None])
def test_paths_are_perft(name, depth, count):
    fen = rc.ROOT_FEN[name]
    got = rc.paths(fen, depth)
    assert len(got) == count == ch.Board(fen).perft(depth)
    assert len({tuple(p[:depth]) for p in got}) == count
    assert all(depth <= len(p) <= depth + 1 for p in got)               # none of these roots is mated within `depth` plies


def test_paths_stop_at_mate_and_extend_otherwise():
    fen = "7k/8/5K2/6Q1/8/8/8/8 w - - 0 1"                               # Qg7 mates at once, Qg6 stalemates; other lines go on
    got = rc.expected(fen, 2)
    short = [u for u, _, _ in got if len(u) == 1]
    assert sorted(short) == [("g5g6",), ("g5g7",)] and len({u[:2] for u, _, _ in got}) == len(got)
    root = ch.Board(fen)
    replies = 0
    for m in root.legal_moves:
        root.push(m)
        replies += max(1, len(root.legal_moves))
        root.pop()
    assert len(got) == replies
    for u, rows, end in got:
        b = ch.Board(fen)
        for k, m in enumerate(u):
            assert rows[k] == (len(b.legal_moves), ch.move_to_index(b, ch.Move.from_uci(m)), int(b.turn), ru.raw_move(m))
            b.push(ch.Move.from_uci(m))
        assert end == {"checkmate": b.is_checkmate(), "stalemate": b.is_stalemate(),
                       "insufficient": b.is_insufficient_material(), "white_to_move": bool(b.turn)}
        assert len(u) == 3 or not b.legal_moves                          # shorter only where the game is over
    assert rc.paths(fen, 2) == [list(u) for u, _, _ in got]


def test_host_core_equals_the_oracle_on_the_whole_neighbourhood():
    """hc_legal (scalar gen_legal of csrc/chess_core.h): moves, order, policy indices; the two-phase generator the tree kernels
    run one move per lane; encode_board."""
    shim = host_shim.load("chess")
    mv, idx, mv2 = (C.c_int32 * 256)(), (C.c_int32 * 256)(), (C.c_int32 * 256)()
    planes = np.zeros((19, 8, 8), np.float32)
    for fen in rc.neighbourhood(2):
        b = ch.Board(fen)
        moves, idxs = ch.legal_moves_with_indices(b)
        n = shim.hc_legal(fen.encode(), mv, idx)
        assert n == len(moves), fen
        assert [(mv[i] & 255, (mv[i] >> 8) & 255, (mv[i] >> 16) or None) for i in range(n)] == \
            [(m.from_square, m.to_square, m.promotion) for m in moves], fen
        assert idx[:n] == idxs, fen
        assert shim.hc_legal_two_phase(fen.encode(), mv2) == n and mv2[:n] == mv[:n], fen
        assert shim.hc_encode(fen.encode(), planes.ctypes.data_as(C.c_void_p)) == 0
        assert np.array_equal(planes, ch.encode_board(b)), fen


def test_host_replay_refuses_what_is_not_legal():
    """What tests/test_rules_edges_gpu.py asks of the device, asked of the host build of the same matching rule."""
    n_bad = n_good = 0
    for _, _, fen in rc.ROOTS:
        bad, good = rc.refusals(fen)
        assert sorted(good) == sorted(m.uci() for m in ch.Board(fen).legal_moves) and not set(bad) & set(good)
        for u in bad:
            r = ru.shim_replay(fen, [u], "uci")
            assert (r["status"], r["plies"]) == ("illegal", 0), (fen, u)
        for u in good:
            r = ru.shim_replay(fen, [u], "uci")
            assert (r["status"], r["plies"]) == ("ok", 1) and r["moves"].tolist() == [ru.raw_move(u)], (fen, u)
        n_bad, n_good = n_bad + len(bad), n_good + len(good)
    assert n_bad > 20000 and n_good > 2000


def test_host_decode_takes_every_position_back():
    """decode_planes_host (csrc/planes_decode.h) on the oracle's planes and masks of the neighbourhood: accepted, the oracle's
    legal count, the en-passant square from the mask exactly where a capture is legal, the oracle's FEN."""
    from tests import planes_cases as pc
    nb = rc.neighbourhood(2)
    planes, mask = np.zeros((len(nb), 19, 8, 8), np.float32), np.zeros((len(nb), 4672), np.uint8)
    boards = [ch.Board(f) for f in nb]
    for i, b in enumerate(boards):
        planes[i], mask[i] = ch.encode_board(b), ch.get_legal_actions(b)
    d = pc.host_decode(planes, mask)
    assert not d["status"].any() and d["nlegal"].tolist() == [len(b.legal_moves) for b in boards]
    for b, fen, flags, got in zip(boards, nb, d["flags"], d["fens"]):
        assert bool(flags & pc.EP_FROM_MASK) == any(rc.is_en_passant(b, m) for m in b.legal_moves), fen
        assert not flags & ~pc.EP_FROM_MASK and got == b.fen(), (fen, got)


def test_host_replay_equals_the_oracle_on_every_path():
    games, want = rc.replay_set()
    assert 30000 <= len(games) <= 60000
    for (fen, ucis), (rows, end) in zip(games, want):
        r = ru.shim_replay(fen, ucis, "uci")
        assert r["status"] == "ok" and r["plies"] == len(ucis) == len(rows), (fen, ucis)
        assert r["end"] == end, (fen, ucis)
        got = list(zip(r["nlegal"].tolist(), r["policy_idx"].tolist(), r["turn"].tolist(), r["moves"].tolist()))
        assert got == list(rows), (fen, ucis)
