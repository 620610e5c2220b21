"""Shared by tests/test_game_import.py and tests/test_game_import_gpu.py: the host shim of the replay
(tests/host_shim/replay_shim.cpp: san_match.h and a scalar replay over gen_legal, compiled by g++), wrapped to answer like
matrix0_amd.game_import.replay_games, the fixture games, and the hand-made cases with their expected outcome."""
import ctypes as C
import functools
import gzip
import json
import os

import numpy as np

from tests import host_shim

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "eval_games_san.json.gz")
STATUS = {0: "ok", 1: "illegal", 2: "ambiguous", 3: "too_long"}
FIELDS = ("kind", "type", "from_file", "from_rank", "to", "promo", "valid")
KIND_SAN, KIND_SHORT, KIND_LONG, KIND_EXACT = 0, 1, 2, 3
PAWN, KNIGHT, BISHOP, ROOK, QUEEN, KING = range(6)


def shim():
    return host_shim.load("replay")


@functools.lru_cache(maxsize=None)
def fixture_games():
    """[(tokens, result header)] of the reference's 125 evaluation games."""
    return [(list(t), r) for t, r in json.load(gzip.open(GOLD, "rt"))]


def square(name):
    return (ord(name[0]) - 97) + 8 * (int(name[1]) - 1)


def raw_move(uci):
    return square(uci[:2]) | (square(uci[2:4]) << 6) | ((" nbrq".index(uci[4]) if len(uci) > 4 else 0) << 12)


def shim_pattern(token, notation="san"):
    """(rc, pattern) of the host parser for a SAN / UCI string or a raw integer move."""
    out = C.c_uint32(0)
    if not isinstance(token, str):
        rc = shim().rs_raw_pattern(int(token), C.byref(out))
    elif notation == "san":
        rc = shim().rs_san_pattern(token.encode(), C.byref(out))
    else:
        rc = shim().rs_uci_pattern(token.encode(), C.byref(out))
    return rc, int(out.value)


def pattern_fields(pat):
    f = np.zeros(7, np.int32)
    shim().rs_pattern_fields(pat, f.ctypes.data_as(C.c_void_p))
    return dict(zip(FIELDS, f.tolist()))


def shim_replay(fen, tokens, notation="san", max_plies=1024, planes=False):
    """One game on the host shim, in the shape replay_games gives (no mask, no ssl; planes on request)."""
    n = len(tokens)
    pats = np.array([shim_pattern(t, notation)[1] for t in tokens], np.uint32).reshape(n)
    rows = max(n, 1)
    out = {"moves": np.zeros(rows, np.uint16), "policy_idx": np.zeros(rows, np.int32), "nlegal": np.zeros(rows, np.int32),
           "turn": np.zeros(rows, np.int8)}
    pl = np.zeros((rows, 19, 8, 8), np.float32) if planes else None
    plies, status, end = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None   # noqa: E731
    rc = shim().rs_replay(fen.encode() if fen else None, p(pats) if n else None, n, max_plies, p(out["moves"]), p(out["policy_idx"]),
                          p(out["nlegal"]), p(out["turn"]), p(pl), C.byref(plies), C.byref(status), C.byref(end))
    assert rc == 0, fen
    res = {k: v[:n] for k, v in out.items()}
    if planes:
        res["planes"] = pl[:n]
    res.update(status=STATUS[status.value], plies=plies.value,
               end={"checkmate": bool(end.value & 1), "stalemate": bool(end.value & 2), "insufficient": bool(end.value & 4),
                    "white_to_move": bool(end.value & 8)})
    return res


def fake_replay_games(games, *, notation="san", ssl=False, planes=True, mask=True, device_index=0, max_plies=1024,
                      max_positions_per_launch=16384):
    """Stands in for game_import.replay_games where there is no GPU: the shim's answers, the shim's planes, and a mask that holds
    the played move only."""
    res = []
    for fen, toks in games:
        r = shim_replay(fen, toks, notation, max_plies, planes=planes)
        n = len(toks)
        if mask:
            r["mask"] = np.zeros((n, 4672), np.uint8)
            r["mask"][np.arange(r["plies"]), r["policy_idx"][: r["plies"]]] = 1
        if ssl:
            r["ssl"] = np.zeros((n, 17, 8, 8), np.float32)
        res.append(r)
    return res


PIN_FEN = "4k3/1b6/8/8/8/5N2/8/1N5K w - - 0 1"          # the f3 knight is pinned by the b7 bishop against the king on h1
# name -> (start FEN or None, tokens, max_plies, expected status, expected plies, expected moves of the resolved prefix)
HAND_CASES = {
    "en_passant": ("rnbqkbnr/ppp1p1pp/8/3pPp2/8/8/PPPP1PPP/RNBQKBNR w KQkq f6 0 3", ["exf6", "exf6"], 1024, "ok", 2, ["e5f6", "e7f6"]),
    "two_knights_ambiguous": ("4k3/8/8/8/8/5N2/8/1N2K3 w - - 0 1", ["Nd2"], 1024, "ambiguous", 0, []),
    "one_knight_pinned": (PIN_FEN, ["Nd2"], 1024, "ok", 1, ["b1d2"]),
    "pinned_piece_moves": (PIN_FEN, ["Ne5"], 1024, "illegal", 0, []),
    "castle_through_check": ("5r2/4k3/8/8/8/8/8/4K2R w K - 0 1", ["O-O"], 1024, "illegal", 0, []),
    "black_to_move_start": ("rnbqkbnr/pppppppp/8/8/4P3/8/PPPP1PPP/RNBQKBNR b KQkq e3 0 1", ["e5", "Nf3", "Nc6"], 1024, "ok", 3,
                            ["e7e5", "g1f3", "b8c6"]),
    "over_specified": (None, ["Ngf3", "e5", "Nb1c3"], 1024, "ok", 3, ["g1f3", "e7e5", "b1c3"]),
    "stops_in_the_middle": (None, ["e4", "e5", "Ke3", "Nc6"], 1024, "illegal", 2, ["e2e4", "e7e5"]),
    "castles": ("r3k2r/8/8/8/8/8/8/R3K2R w KQkq - 0 1", ["0-0", "O-O-O+"], 1024, "ok", 2, ["e1g1", "e8c8"]),
    "king_step_is_no_castle": ("r3k2r/8/8/8/8/8/8/R3K2R w KQkq - 0 1", ["Kg1"], 1024, "illegal", 0, []),
    "too_long": (None, None, 10, "too_long", 10, None),     # tokens: fixture game 0
}


def hand_case(name):
    fen, toks, max_plies, status, plies, moves = HAND_CASES[name]
    if toks is None:
        toks = fixture_games()[0][0]
    return fen, toks, max_plies, status, plies, moves
