"""Shared by tests/test_rules_cases.py (CPU) and tests/test_rules_edges_gpu.py: root positions at the edges of the chess rules, each
named and filed under the class it stands for, and what the oracle says about the positions and the move sequences around them.

neighbourhood(depth) gives the unique positions within `depth` plies of the roots, paths(root, depth) every legal move sequence of
that length (perft, with the moves written out), expected(root, depth) the oracle's rows for those sequences.  Everything here is
computed with oracle/chess_py.py when it is first asked for, kept for the process and never modified."""
import functools

from oracle import chess_py as ch


def mirror(fen):
    """The same position with the colours swapped (ranks flipped, side to move, castling rights and en-passant square with them)."""
    board, turn, castling, ep, half, full = fen.split(" ")
    board = "/".join(r.swapcase() for r in reversed(board.split("/")))
    castling = "-" if castling == "-" else "".join(sorted(castling.swapcase(), key="KQkq".index))
    ep = "-" if ep == "-" else ep[0] + str(9 - int(ep[1]))
    return " ".join([board, "b" if turn == "w" else "w", castling, ep, half, full])


KIWIPETE = "r3k2r/p1ppqpb1/bn2pnp1/3PN3/1p2P3/2N2Q1p/PPPBBPPP/R3K2R w KQkq - 0 1"
PERFT3 = "8/2p5/3p4/KP5r/1R3p1k/8/4P1P1/8 w - - 0 1"
PERFT4 = "r3k2r/Pppp1ppp/1b3nbN/nP6/BBP1P3/q4N2/Pp1P2PP/R2Q1RK1 w kq - 0 1"
PERFT5 = "rnbq1k1r/pp1Pbppp/2p5/8/2B5/8/PPP1NnPP/RNBQK2R w KQ - 1 8"
PERFT6 = "r4rk1/1pp1qppp/p1np1n2/2b1p1B1/2B1P1b1/P1NP1N2/1PP1QPPP/R4RK1 w - - 0 10"
PROMOTIONS = "n1n5/PPPk4/8/8/8/8/4Kppp/5N1N b - - 0 1"
WIDE_218 = "R6R/3Q4/1Q4Q1/4Q3/2Q4Q/Q4Q2/pp1Q4/kBNN1KB1 w - - 0 1"
WIDE_218_B = "3Q4/1Q4Q1/4Q3/2Q4R/Q4Q2/3Q4/1Q4Rp/1K1BBNNk w - - 0 1"
WIDE_138 = "1Q2Q3/Q6Q/8/3k4/8/Q6Q/1Q2Q3/4K3 w - - 0 1"
# legal-move count -> a root with exactly that many: the sizes at which "child i = lane + 64 k" takes one more round
WAVE_EDGE = {
    63: "8/6Q1/1Q6/7k/1K6/8/8/R7 w - - 0 1",
    64: "1K6/8/8/5Q2/1B6/4Q3/8/3k4 w - - 0 1",
    65: "8/8/3k2K1/QQ6/8/2Q5/8/8 w - - 0 1",
    127: "6QQ/1k6/8/1K2Q2Q/2Q5/1QQ3N1/3Q4/1Q1BN3 w - - 0 1",
    128: "3k4/1Q4Q1/4K3/8/Q4Q2/6N1/Q5Q1/4Q3 w - - 0 1",
    129: "Q4KN1/7k/Q7/2Q5/3Q1Q2/2Q5/1Q3Q2/8 w - - 0 1",
}

# the castling roots are written for White, all with both rights in the FEN, and stand in the corpus a second time with the colours
# swapped: (name, class, FEN, the castles the rules leave: "g" short, "c" long)
_CASTLING = [
    ("castle_b_file_attacked", "castle_allowed_b_attacked", "1r2k3/8/8/8/8/8/8/R3K2R w KQ - 0 1", "gc"),
    ("castle_transit_attacked", "castle_refused_transit", "3r1r2/6k1/8/8/8/8/8/R3K2R w KQ - 0 1", ""),
    ("castle_destination_attacked", "castle_refused_destination", "2r3r1/5k2/8/8/8/8/8/R3K2R w KQ - 0 1", ""),
    ("castle_in_check", "castle_refused_in_check", "4r3/6k1/8/8/8/8/8/R3K2R w KQ - 0 1", ""),
    ("castle_b_file_blocked", "castle_refused_b_blocked", "4k3/8/8/8/8/8/8/RN2K2R w KQ - 0 1", "g"),
    ("castle_right_without_rook", "castle_refused_no_rook", "4k3/8/8/8/8/8/8/N3K2R w KQ - 0 1", "g"),
    ("castle_king_off_its_square", "castle_refused_king_moved", "4k3/8/8/8/8/8/8/R2K3R w KQ - 0 1", ""),
]

# (name, class, FEN)
ROOTS = [
    # ---- en passant ----
    ("ep_legal_white", "ep_legal", "rnbqkbnr/ppp1p1pp/8/3pPp2/8/8/PPPP1PPP/RNBQKBNR w KQkq f6 0 3"),
    ("ep_legal_black", "ep_legal", "rnbqkbnr/pppp1ppp/8/8/3Pp3/8/PPP1PPPP/RNBQKBNR b KQkq d3 0 3"),
    ("ep_both_pawns_leave_the_rank_white", "ep_illegal_rank", "8/8/8/KPp4r/8/8/8/7k w - c6 0 2"),
    ("ep_both_pawns_leave_the_rank_black", "ep_illegal_rank", "7K/8/8/8/R4pPk/8/8/8 b - g3 0 1"),
    ("ep_capturer_pinned_on_file", "ep_illegal_pinned_file", "4r2k/8/8/3pP3/8/8/8/4K3 w - d6 0 1"),
    ("ep_capturer_pinned_on_diagonal", "ep_illegal_pinned_diagonal", "7b/8/8/3pP3/8/8/1K6/7k w - d6 0 1"),
    ("ep_capturer_moves_along_its_pin", "ep_legal", "7b/8/8/4Pp2/8/8/1K6/7k w - f6 0 1"),
    ("ep_captured_pawn_shields_diagonal", "ep_illegal_shield_diagonal", "6b1/8/8/3pP3/8/8/K7/7k w - d6 0 1"),
    ("ep_removes_checking_pawn_white", "ep_removes_checker", "8/8/8/3pP3/4K3/8/8/7k w - d6 0 1"),
    ("ep_removes_checking_pawn_black", "ep_removes_checker", "8/8/8/3k4/3pP3/8/8/4K3 b - e3 0 1"),
    # the position the issue files under "removes a checking pawn": the d4 pawn stands beside the king's file and gives no check
    ("ep_pawn_in_front_of_king", "ep_legal", "8/8/8/3k4/2pP4/8/8/4K3 b - d3 0 1"),
    ("ep_two_capturers_white", "ep_two_capturers", "rnbqkbnr/ppppp1pp/8/4PpP1/8/8/PPPP1P1P/RNBQKBNR w KQkq f6 0 4"),
    ("ep_two_capturers_black", "ep_two_capturers", "rnbqkbnr/pp1p1ppp/8/8/2pPp3/8/PPP1PPPP/RNBQKBNR b KQkq d3 0 4"),
    ("ep_square_without_capturer", "ep_no_capturer", "rnbqkbnr/pppppppp/8/8/4P3/8/PPPP1PPP/RNBQKBNR b KQkq e3 0 1"),
    ("ep_blocks_a_bishop_check", "ep_in_check", "7k/b7/8/Pp6/8/8/8/6K1 w - b6 0 1"),
    ("ep_no_answer_to_a_rook_check", "ep_in_check", "r6k/8/8/3pP3/8/8/8/K7 w - d6 0 1"),
    # ---- check ----
    ("double_check", "double_check", "4k3/8/8/8/8/5n2/6B1/3QK2r w - - 0 1"),
    ("double_check_ahead_white", "before_double_check", "4k3/8/8/8/4N3/8/8/4RK2 w - - 0 1"),
    ("double_check_ahead_black", "before_double_check", "4rk2/8/8/4n3/8/8/8/4K3 b - - 0 1"),
    ("check_capture_with_promotion", "check_answers", "3r3k/2P5/8/8/8/8/8/3K4 w - - 0 1"),
    ("check_block_with_promotion", "check_answers", "K6r/3P4/8/8/8/8/8/7k w - - 0 1"),
    ("check_block_capture_or_step", "check_answers", "4r2k/8/8/8/8/2N5/3B4/R3K3 w - - 0 1"),
    ("check_everything_pinned", "check_all_pinned", "4r2k/8/8/b7/7b/3n4/3BRN2/4K3 w - - 0 1"),
    # ---- promotion ----
    ("promotion_white_push_and_captures", "promotion", "1n1n3k/2P5/8/8/8/8/8/K7 w - - 0 1"),
    ("promotion_black_push_and_captures", "promotion", "k7/8/8/8/8/8/2p5/1N1N3K b - - 0 1"),
    ("promotion_pawn_pinned_on_diagonal", "promotion_pinned", "2n1b2k/3P4/8/8/K7/8/8/8 w - - 0 1"),
    ("promotion_pawn_pinned_on_rank", "promotion_pinned", "2n1n2k/1K1P3r/8/8/8/8/8/8 w - - 0 1"),
    ("promotions_both_sides", "promotion", PROMOTIONS),
    # ---- wide ----
    ("wide_218", "wide", WIDE_218),
    ("wide_218_second", "wide", WIDE_218_B),
    ("wide_138", "wide", WIDE_138),
    ("wide_138_black", "wide", mirror(WIDE_138)),
] + [(f"wide_{n}", "wave_edge", fen) for n, fen in WAVE_EDGE.items()] + [
    # ---- terminal ----
    ("stalemate", "terminal", "7k/5Q2/6K1/8/8/8/8/8 b - - 0 1"),
    ("checkmate_back_rank", "terminal", "R5k1/5ppp/8/8/8/8/8/6K1 b - - 0 1"),
    ("checkmate_fools", "terminal", "rnb1kbnr/pppp1ppp/8/4p3/6Pq/5P2/PPPPP2P/RNBQKBNR w KQkq - 1 3"),
    # ---- perft ----
    ("perft_start", "perft", ch.START_FEN),
    ("perft_kiwipete", "perft", KIWIPETE),
    ("perft_3", "perft", PERFT3),
    ("perft_4", "perft", PERFT4),
    ("perft_4_mirror", "perft", mirror(PERFT4)),
    ("perft_5", "perft", PERFT5),
    ("perft_6", "perft", PERFT6),
]
CASTLES_LEFT = {}                                       # root name -> the castling moves that are legal there
for _name, _cls, _fen, _left in _CASTLING:
    ROOTS.append((_name + "_white", _cls, _fen))
    ROOTS.append((_name + "_black", _cls, mirror(_fen)))
    CASTLES_LEFT[_name + "_white"] = sorted("e1" + f + "1" for f in _left)
    CASTLES_LEFT[_name + "_black"] = sorted("e8" + f + "8" for f in _left)

CLASSES = sorted({c for _, c, _ in ROOTS})
ROOT_FEN = {name: fen for name, _, fen in ROOTS}
assert len(ROOT_FEN) == len(ROOTS) and len(set(ROOT_FEN.values())) == len(ROOTS)

# (root name, depth, published perft count or None): the move sequences the replay tests run
PERFT_PATHS = [("perft_start", 3, 8902), ("perft_3", 3, 2812), ("perft_4", 3, 9467), ("perft_4_mirror", 3, 9467),
               ("promotions_both_sides", 3, 9483), ("perft_kiwipete", 2, 2039), ("perft_5", 2, 1486), ("wide_218", 2, None)]


def fen_raw(b):
    """FEN with the raw en-passant square: set after every double push, whether or not a capture is legal."""
    f = b.fen().split(" ")
    if b.ep_square is not None:
        f[3] = ch.square_name(b.ep_square)
    return " ".join(f)


def is_en_passant(b, m):
    """A pawn that moves diagonally to an empty square."""
    return b.piece_type_at(m.from_square) == ch.PAWN and (m.from_square & 7) != (m.to_square & 7) and \
        not b.piece_code_at(m.to_square)


def pseudo_en_passant(b):
    """The en-passant captures the pawns' geometry allows, legal or not: [(from, to)]."""
    ep = b.ep_square
    if ep is None:
        return []
    own = ch.PAWN if b.turn else ch.PAWN + 6                  # piece codes: white 1..6, black 7..12
    back = -8 if b.turn else 8
    if b.piece_code_at(ep) or b.piece_code_at(ep + back) != (ch.PAWN + 6 if b.turn else ch.PAWN):
        return []
    return [(ep + back + d, ep) for d in (-1, 1) if 0 <= (ep & 7) + d < 8 and b.piece_code_at(ep + back + d) == own]


def checkers(b):
    """The squares of the enemy pieces that attack the king of the side to move.  Each is tried alone: the others, kings apart, are
    turned into knights of the side to move, which block the same lines and check nobody."""
    if not b.is_check():
        return []
    pm = b.piece_map()
    turn = "w" if b.turn else "b"
    out = []
    for sq, code in pm.items():
        if (code <= 6) == b.turn or (code - 1) % 6 + 1 == ch.KING:
            continue
        rows = []
        for r in range(7, -1, -1):
            row = ""
            for f in range(8):
                c = pm.get(r * 8 + f)
                if c is None:
                    row += "1"
                elif r * 8 + f == sq or (c <= 6) == b.turn or (c - 1) % 6 + 1 == ch.KING:
                    row += "PNBRQKpnbrqk"[c - 1]
                else:
                    row += "N" if b.turn else "n"
            rows.append(row)
        if ch.Board(f"{'/'.join(rows)} {turn} - - 0 1").is_check():
            out.append(sq)
    return out


@functools.lru_cache(maxsize=None)
def neighbourhood(depth):
    """The unique positions within `depth` plies of the roots, as raw-en-passant FENs, roots first, in the order a breadth-first
    walk over the roots in corpus order meets them."""
    seen, layer = {}, []
    for _, _, fen in ROOTS:
        f = fen_raw(ch.Board(fen))
        if f not in seen:
            seen[f] = None
            layer.append(f)
    for _ in range(depth):
        nxt = []
        for f in layer:
            b = ch.Board(f)
            for m in b.legal_moves:
                b.push(m)
                g = fen_raw(b)
                b.pop()
                if g not in seen:
                    seen[g] = None
                    nxt.append(g)
        layer = nxt
    return tuple(seen)


def raw_move(m):
    return m.from_square | (m.to_square << 6) | ((m.promotion - 1 if m.promotion else 0) << 12)


def _end(b):
    return {"checkmate": b.is_checkmate(), "stalemate": b.is_stalemate(), "insufficient": b.is_insufficient_material(),
            "white_to_move": bool(b.turn)}


@functools.lru_cache(maxsize=None)
def expected(root, depth):
    """Every legal move sequence of `depth` plies from the FEN `root`, in generation order, each extended by the first legal move
    of the position it reaches (so that position is a row too); a sequence that meets mate or stalemate earlier stops there.
    [(ucis, rows, end)]: rows = one (nlegal, policy index, turn, raw move) per ply for the position BEFORE it, end = the flags
    of the position after the last ply, as game_import.replay_games reports them."""
    out = []
    b = ch.Board(root)
    ucis, rows = [], []

    def leaf():
        moves, idxs = ch.legal_moves_with_indices(b)
        if not moves:
            return (), (), _end(b)
        b.push(moves[0])
        end = _end(b)
        b.pop()
        return (moves[0].uci(),), ((len(moves), idxs[0], int(b.turn), raw_move(moves[0])),), end

    def walk(d):
        if d == depth:
            u, r, end = leaf()
            out.append((tuple(ucis) + u, tuple(rows) + r, end))
            return
        moves, idxs = ch.legal_moves_with_indices(b)
        if not moves:
            out.append((tuple(ucis), tuple(rows), _end(b)))
            return
        turn = int(b.turn)
        for m, i in zip(moves, idxs):
            ucis.append(m.uci())
            rows.append((len(moves), i, turn, raw_move(m)))
            b.push(m)
            walk(d + 1)
            b.pop()
            ucis.pop()
            rows.pop()

    walk(0)
    return tuple(out)


def paths(root, depth):
    """The move sequences of expected(root, depth) alone: a list of lists of UCI strings."""
    return [list(u) for u, _, _ in expected(root, depth)]


@functools.lru_cache(maxsize=None)
def replay_set():
    """All of PERFT_PATHS as one list of games: [(start FEN, ucis)], and beside it the oracle's (rows, end) per game."""
    games, want = [], []
    for name, depth, _ in PERFT_PATHS:
        for u, rows, end in expected(ROOT_FEN[name], depth):
            games.append((ROOT_FEN[name], list(u)))
            want.append((rows, end))
    return games, want


def refusals(fen):
    """One-token games on `fen` that must be refused, and those that must be played: (illegal ucis, legal ucis).  Illegal: every
    from-to pair (from == to among them) whose from-square holds a piece of the side to move and
    which is no legal move, with each of the four promotion suffixes as well where a pawn stands on its seventh rank."""
    b = ch.Board(fen)
    legal = [m.uci() for m in b.legal_moves]
    have = set(legal)
    bad = []
    for sq, code in sorted(b.piece_map().items()):
        if (code <= 6) != b.turn:
            continue
        seventh = (code - 1) % 6 + 1 == ch.PAWN and (sq >> 3) == (6 if b.turn else 1)
        for to in range(64):
            for suffix in ("", "n", "b", "r", "q") if seventh else ("",):
                u = ch.square_name(sq) + ch.square_name(to) + suffix
                if u not in have:
                    bad.append(u)
    return bad, legal
