"""Shared helpers of the tests of the tablebases inside the search: the probe and the analysis of a root inside the tables
once more in Python, over the independent generator's tables (tests/tb_util.py::ref_tables) and the oracle's rules
(oracle/chess_py.py: legal moves, their order, checkmate).  Nothing here calls the library.

A position is looked up from its men, ((square, oracle piece code), ...) in square order, and the side to move; the men after
a move are worked out here (a capture removes the man on the target square, a promotion changes the type), which is all that
can happen without castling rights and with too few pawns for en passant."""
from oracle import chess_py as ch
from tests import tb_util as tu

LETTER = {1: "P", 2: "N", 3: "B", 4: "R", 5: "Q"}      # the oracle's piece types; 6 = king; Black's codes are + 6


def men_of(board: ch.Board):
    return tuple((s, c) for s, c in enumerate(bytes(board._p.contents.sq)) if c)


def has_rights(board: ch.Board) -> bool:
    return any(f(col) for col in (True, False) for f in (board.has_kingside_castling_rights, board.has_queenside_castling_rights))


def locate(men, white_to_move: bool):
    """(signature, index) of csrc/tb_core.h's contract, restated."""
    w, b, wk, bk = [], [], -1, -1
    for s, c in men:
        t = (c - 1) % 6 + 1
        if t == 6:
            if c <= 6:
                wk = s
            else:
                bk = s
        else:
            (w if c <= 6 else b).append((-t, s))
    stm = 0 if white_to_move else 1
    w.sort()                                           # Q > R > B > N > P, identical men by ascending square
    b.sort()
    if (len(b), [-t for t, _ in b]) > (len(w), [-t for t, _ in w]):      # Black is the greater side: the colour flip
        w, b = sorted((t, s ^ 56) for t, s in b), sorted((t, s ^ 56) for t, s in w)
        wk, bk = bk ^ 56, wk ^ 56
        stm ^= 1
    sig = "K" + "".join(LETTER[-t] for t, _ in w) + "K" + "".join(LETTER[-t] for t, _ in b)
    idx, sh = wk, 6
    for _, s in w:
        idx |= s << sh
        sh += 6
    idx |= bk << sh
    sh += 6
    for _, s in b:
        idx |= s << sh
        sh += 6
    return sig, idx | (stm << sh)


def lookup(men, white_to_move: bool, tables: dict, max_men: int = 3):
    """(wdl for the side to move, dtm in plies) or None: more than max_men men, no table of the material, an invalid entry."""
    if len(men) > max_men:
        return None
    sig, idx = locate(men, white_to_move)
    table = tables.get(sig)
    if table is None:
        return None
    v = int(table[idx])
    return None if v == 255 else tu.entry_wdl_dtm(v)


def py_probe(board: ch.Board, tables: dict, max_men: int = 3):
    """The probe of a board: no hit also with a castling right left."""
    men = men_of(board)
    if len(men) > max_men or has_rights(board):
        return None
    return lookup(men, board.turn, tables, max_men)


def men_after(men, m: ch.Move):
    out = []
    for s, c in men:
        if s == m.to_square:
            continue                                   # captured
        if s == m.from_square:
            out.append((m.to_square, (m.promotion + (0 if c <= 6 else 6)) if m.promotion else c))
        else:
            out.append((s, c))
    return tuple(out)


def ranked_moves(board: ch.Board, tables: dict, max_men: int = 3):
    """[(move, wdl, dtm of the successor)] best first for the mover: successors lost for the opponent by ascending dtm, then
    drawn ones, then successors won for the opponent by descending dtm; ties in legal-move order.  `board` has no castling
    rights."""
    men, out = men_of(board), []
    for m in board.legal_moves:
        hit = lookup(men_after(men, m), not board.turn, tables, max_men)
        assert hit is not None, (board.fen(), m.uci())
        out.append((m, hit[0], hit[1]))
    out.sort(key=lambda r: (0, r[2]) if r[1] < 0 else ((1, 0) if r[1] == 0 else (2, -r[2])))      # stable
    return out


def py_root_lines(fen: str, tables: dict, multipv: int, pv_len: int, max_men: int = 3, best_reply: dict = None):
    """None when `fen` is no hit, else {"root_q", "dtm", "nlegal", "lines": [{"move", "q", "dtm", "pv"}]} as
    m0_tb_root_lines states it.  `best_reply` (optional) remembers the first-ranked move of the positions walked through."""
    if fen.split()[2] != "-":
        return None                                    # a castling right left
    board = ch.Board(fen)
    root = lookup(men_of(board), board.turn, tables, max_men)
    if root is None:
        return None
    ranked = ranked_moves(board, tables, max_men)
    lines = []
    for m, wdl, dtm in ranked[:multipv]:
        pv = [m.uci()]
        if wdl != 0:                                   # a decided line: the first-ranked move of every position on it
            b = board.copy()
            b.push(m)
            while len(pv) < pv_len:
                key = (men_of(b), b.turn)
                if best_reply is not None and key in best_reply:
                    first = best_reply[key]
                else:
                    nxt = ranked_moves(b, tables, max_men)
                    first = nxt[0][0] if nxt else None
                    if best_reply is not None:
                        best_reply[key] = first
                if first is None:
                    break                              # checkmate
                pv.append(first.uci())
                b.push(first)
        lines.append({"move": m.uci(), "q": float(-wdl), "dtm": dtm, "pv": pv})
    return {"root_q": float(root[0]), "dtm": root[1], "nlegal": len(ranked), "lines": lines}
