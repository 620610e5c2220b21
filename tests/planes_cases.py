"""Shared by tests/test_planes_decode.py (CPU) and tests/test_reanalyse_gpu.py: the host build of the planes decode
(tests/host_shim/planes_shim.cpp), the hand-written en-passant positions and one malformed row per decode status."""
import ctypes as C

import numpy as np

from oracle import chess_py as ch
from tests import host_shim

# status codes and flags of include/m0_engine.h
(OK, PIECE_VALUE, SQUARE_CLASH, KINGS, PAWN_RANK, NOT_UNIFORM, FLAG_VALUE, CASTLING, COUNTER, OPPONENT_IN_CHECK, TOO_MANY_MOVES,
 MASK_MISMATCH) = range(12)
HALFMOVE_SATURATED, FULLMOVE_SATURATED, EP_FROM_MASK, NO_MASK = 1, 2, 4, 8

# (fen, the en-passant square a decode WITH the mask must recover or None)
EP_FENS = [
    ("rnbqkbnr/ppp1p1pp/8/3pPp2/8/8/PPPP1PPP/RNBQKBNR w KQkq f6 0 3", "f6"),       # White captures
    ("rnbqkbnr/pppp1ppp/8/8/3Pp3/8/PPP1PPPP/RNBQKBNR b KQkq d3 0 3", "d3"),        # Black captures
    ("rnbqkbnr/ppppp1pp/8/4PpP1/8/8/PPPP1P1P/RNBQKBNR w KQkq f6 0 4", "f6"),       # two white pawns can both capture
    ("rnbqkbnr/pp1p1ppp/8/8/2pPp3/8/PPP1PPPP/RNBQKBNR b KQkq d3 0 4", "d3"),       # two black pawns can both capture
    ("rnbqkbnr/1ppppppp/8/pP6/8/8/P1PPPPPP/RNBQKBNR w KQkq a6 0 3", "a6"),         # on the a-file
    ("rnbqkbnr/pppppp1p/8/8/6pP/8/PPPPPPP1/RNBQKBNR b KQkq h3 0 3", "h3"),         # on the h-file
    ("8/8/8/3pP3/4K3/8/8/7k w - d6 0 1", "d6"),                                    # the capture removes the checking pawn
    ("8/8/8/K2pP2r/8/8/8/7k w - d6 0 1", None),                                    # illegal: both pawns leave the rank, the rook checks
    ("4r2k/8/8/3pP3/8/8/8/4K3 w - d6 0 1", None),                                  # illegal: the pawn is pinned on the file
    ("7K/8/8/8/k2Pp2R/8/8/8 b - d3 0 1", None),                                    # illegal for Black, the same way
    ("rnbqkbnr/pppppppp/8/8/4P3/8/PPPP1PPP/RNBQKBNR b KQkq e3 0 1", None),         # a double push with no enemy pawn beside it
    ("rnbqkbnr/pppp1ppp/8/4p3/4P3/8/PPPP1PPP/RNBQKBNR w KQkq e6 0 2", None),
    ("rnbqkbnr/ppp1pppp/8/3pP3/8/8/PPPP1PPP/RNBQKBNR w KQkq - 0 3", None),         # the pawns stand so, but it was no double push
]


def host_decode(planes, mask=None):
    """decode_planes_host (csrc/planes_decode.h) over rows: status, flags, nlegal, fens and, for the rows that left a position,
    its legal moves (raw u16) with their policy indices in generation order and its planes encoded again."""
    pl = np.ascontiguousarray(planes, np.float32)
    n = pl.shape[0]
    mk = None if mask is None else np.ascontiguousarray(np.asarray(mask).reshape(n, -1), np.uint8)
    status, flags, nlegal = (np.zeros(n, np.int32) for _ in range(3))
    stride = 96
    fens = C.create_string_buffer(max(1, n) * stride)
    moves, idx = np.zeros((n, 256), np.uint16), np.full((n, 256), -1, np.int32)
    again = np.zeros((n, 19, 8, 8), np.float32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = host_shim.load("planes").pd_decode(ptr(pl), ptr(mk) if mk is not None else None, n, ptr(status), ptr(flags),
                                            ptr(nlegal), fens, stride, ptr(moves), ptr(idx), ptr(again))
    assert rc == 0
    raw = fens.raw
    return {"status": status, "flags": flags, "nlegal": nlegal, "moves": moves, "idx": idx, "planes": again,
            "fens": [raw[i * stride: (i + 1) * stride].split(b"\0", 1)[0].decode() for i in range(n)]}


def encode(fen):
    """(planes f32 [19,8,8], mask u8 [4672]) of a FEN by the oracle: what a stored row of that position holds."""
    b = ch.Board(fen)
    return ch.encode_board(b), np.asarray(ch.get_legal_actions(b)).astype(np.uint8)


def is_en_passant(board, m):
    """A pawn that moves diagonally to an empty square."""
    return board.piece_type_at(m.from_square) == ch.PAWN and (m.from_square & 7) != (m.to_square & 7) and \
        not board.piece_code_at(m.to_square)


def malformed_rows():
    """[(name, expected status, planes, mask)]: every decode status but OK at least once; the mask is the true one of the
    row's source position unless the case is about the mask."""
    start, start_mask = encode(ch.START_FEN)
    bare, bare_mask = encode("4k3/8/8/8/8/8/4P3/4K3 w - - 0 1")
    rows = []

    def add(name, want, planes, mask):
        rows.append((name, want, np.ascontiguousarray(planes, np.float32), np.ascontiguousarray(mask, np.uint8)))

    for name, v in (("half", 0.5), ("nan", np.nan), ("two", 2.0), ("minus_zero", -0.0), ("denormal", 1e-45)):
        p = start.copy(); p[3, 4, 4] = v
        add("piece_value_" + name, PIECE_VALUE, p, start_mask)
    p = start.copy(); p[1, 6, 0] = 1.0                          # a white knight on the a2 pawn
    add("clash", SQUARE_CLASH, p, start_mask)
    p = start.copy(); p[6, 6, 0] = 1.0                          # a black pawn on it
    add("clash_colours", SQUARE_CLASH, p, start_mask)
    p = start.copy(); p[5] = 0.0
    add("no_white_king", KINGS, p, start_mask)
    p = start.copy(); p[11, 4, 4] = 1.0
    add("two_black_kings", KINGS, p, start_mask)
    p = bare.copy(); p[0, 6, 4] = 0.0; p[0, 7, 0] = 1.0         # the pawn from e2 to a1
    add("pawn_rank_1", PAWN_RANK, p, bare_mask)
    p = bare.copy(); p[0, 6, 4] = 0.0; p[6, 0, 7] = 1.0         # a black pawn on h8
    add("pawn_rank_8", PAWN_RANK, p, bare_mask)
    for k in range(12, 19):
        p = start.copy(); p[k, 7, 7] = 0.25
        add(f"not_uniform_{k}", NOT_UNIFORM, p, start_mask)
    p = start.copy(); p[12] = 0.5
    add("turn_half", FLAG_VALUE, p, start_mask)
    p = start.copy(); p[15] = np.nan
    add("castling_nan", FLAG_VALUE, p, start_mask)
    p = bare.copy(); p[13] = 1.0                                # a right without its rook
    add("castling_no_rook", CASTLING, p, bare_mask)
    p = start.copy(); p[5, 7, 4] = 0.0; p[5, 5, 4] = 1.0; p[0, 6, 4] = 0.0; p[0, 4, 4] = 1.0   # Ke3 (pawn to e4): rights left set
    add("castling_king_moved", CASTLING, p, start_mask)
    p = start.copy(); p[17] = 0.5
    add("halfmove_no_k_over_99", COUNTER, p, start_mask)
    p = start.copy(); p[17] = np.nextafter(np.float32(3.0 / 99.0), np.float32(1.0))
    add("halfmove_one_ulp_off", COUNTER, p, start_mask)
    p = start.copy(); p[18] = np.float32(1.5)
    add("fullmove_above_cap", COUNTER, p, start_mask)
    p = start.copy(); p[18] = np.float32(-1.0 / 199.0)
    add("fullmove_negative", COUNTER, p, start_mask)
    p, m = encode("4k3/8/8/8/8/8/8/4RK2 w - - 0 1")             # White to move, Black in check
    add("opponent_in_check", OPPONENT_IN_CHECK, p, m)
    # 24 white queens round the rim and about, the black king walled in: 250-odd legal moves, and a bound beyond the 256 a move
    # list holds (the generators would write past it)
    p, m = encode("kb6/pp6/8/8/8/8/8/K7 w - - 0 1")
    for sq in (1, 2, 3, 4, 5, 6, 7, 8, 15, 16, 23, 24, 28, 32, 39, 40, 41, 47, 54, 58, 59, 60, 61, 62):
        p[4, 7 - sq // 8, sq % 8] = 1.0
    add("board_of_queens", TOO_MANY_MOVES, p, m)
    m = start_mask.copy(); m[int(np.flatnonzero(m == 0)[100])] = 1
    add("mask_extra_bit", MASK_MISMATCH, start, m)
    m = start_mask.copy(); m[int(np.flatnonzero(m)[7])] = 0
    add("mask_missing_bit", MASK_MISMATCH, start, m)
    return rows
