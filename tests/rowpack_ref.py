"""A numpy restatement of the packed training rows, written from the description in include/m0_rowpack.h and sharing no code with
the engine: men from planes 0-11, the scalar fields from round(x * 99) / round(x * 199), the legal columns from oracle.chess_py on
the FEN (en passant included), and unpacking by oracle.chess_py.encode_board.  tests/test_rowpack.py compares the host calls with
it.  The switches of Mutations each break one rule; the tests show that some row then differs."""
from dataclasses import dataclass

import numpy as np

from oracle import chess_py as ch

COLS = 4672
PACKED, RAW = 0, 1
MASK_NONE, MASK_LEGAL, MASK_LIST = 0, 1, 2
ONE = 0x3F800000
PIECES = "PNBRQKpnbrqk"                      # plane order
KNIGHT = [(-2, -1), (-2, 1), (-1, -2), (-1, 2), (1, -2), (1, 2), (2, -1), (2, 1)]
KING = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]
ROOK, BISHOP = [(1, 0), (-1, 0), (0, 1), (0, -1)], [(1, 1), (1, -1), (-1, 1), (-1, -1)]


@dataclass
class Mutations:
    entry_by_value: bool = False             # an entry is pi != 0.0 instead of a non-zero bit pattern: loses -0.0
    drop_ep: bool = False                    # the en-passant square is not stored
    legal_on_mismatch: bool = False          # a mask that differs from the legal moves is still called LEGAL
    # The issue names "castling bits taken before cleaning".  A PACKED row's planes re-encode bit for bit, so their four bits ARE
    # the cleaned ones and bits "before cleaning" do not exist on such a row (planes with a right the men cannot have make the row
    # RAW: tests/planes_cases.py castling_no_rook, castling_king_moved).  What can drift is a packer that takes the rights from
    # somewhere else than the planes; this switch takes them from the men instead -- every right whose king and rook stand at home
    # -- which differs from the planes wherever a right was lost by moving and returning.
    castling_from_men: bool = False


def _f32(x):
    return np.float32(x).view(np.uint32)


def _targets(board, sq, steps, slide, own):
    n, r0, f0 = 0, sq >> 3, sq & 7
    for dr, df in steps:
        r, f = r0 + dr, f0 + df
        while 0 <= r < 8 and 0 <= f < 8:
            t = r * 8 + f
            if t not in own:
                n += 1
            if not slide or t in board:
                break
            r, f = r + dr, f + df
    return n


def moves_bound(board, white):
    """An upper bound of the pseudo-legal moves of {square: plane}: two castlings, two en-passant captures, every piece's targets
    off its own men, pawn captures and pushes (four promotions each on the last rank; every single push may double)."""
    own = {s for s, k in board.items() if (k < 6) == white}
    n = 4
    for s in own:
        t = board[s] % 6
        if t == 0:
            up = 8 if white else -8
            for df in (-1, 1):
                c = s + up + df
                if 0 <= (s & 7) + df < 8 and c in board and c not in own:
                    n += 4 if (c >> 3) in (0, 7) else 1
            if s + up not in board:
                n += (4 if ((s + up) >> 3) in (0, 7) else 1) + 1
        else:
            steps = {1: KNIGHT, 2: BISHOP, 3: ROOK, 4: ROOK + BISHOP, 5: KING}[t]
            n += _targets(board, s, steps, t in (2, 3, 4), own)
    return n


def position_of(planes, mask):
    """None when the planes are no position the packed form may keep; else dict(men u64 [12], turn, castling, ep, halfmove,
    fullmove, legal: the sorted legal columns)."""
    bits = np.ascontiguousarray(planes, np.float32).reshape(19, 8, 8).view(np.uint32)
    men_planes = bits[:12]
    if not np.isin(men_planes, (0, ONE)).all() or ((men_planes == ONE).sum(axis=0) > 1).any():
        return None
    if (bits[12:] != bits[12:, :1, :1]).any() or not np.isin(bits[12:17, 0, 0], (0, ONE)).all():
        return None
    board = {}
    for k, r, f in zip(*np.nonzero(men_planes == ONE)):
        board[(7 - int(r)) * 8 + int(f)] = int(k)
    kinds = list(board.values())
    if kinds.count(5) != 1 or kinds.count(11) != 1 or any(k % 6 == 0 and (s >> 3) in (0, 7) for s, k in board.items()):
        return None
    x17, x18 = planes.reshape(19, 64)[17, 0], planes.reshape(19, 64)[18, 0]
    if not (0.0 <= x17 <= 1.0 and 0.0 <= x18 <= 1.0):
        return None
    half, full = int(round(float(x17) * 99)), int(round(float(x18) * 199))
    if _f32(half / 99.0) != _f32(x17) or _f32(full / 199.0) != _f32(x18):
        return None
    white = bool(bits[12, 0, 0])
    castling = sum(1 << i for i in range(4) if bits[13 + i, 0, 0])
    rows = []
    for r in range(7, -1, -1):
        row, gap = "", 0
        for f in range(8):
            k = board.get(r * 8 + f)
            if k is None:
                gap += 1
            else:
                row, gap = row + (str(gap) if gap else "") + PIECES[k], 0
        rows.append(row + (str(gap) if gap else ""))
    placement = "/".join(rows)
    rights = "".join(c for i, c in enumerate("KQkq") if castling >> i & 1) or "-"
    fen = lambda turn, ep: f"{placement} {'w' if turn else 'b'} {rights} {ep} {half} {full}"
    if ch.Board(fen(not white, "-")).is_check() or moves_bound(board, white) > 256:          # the side that just moved left itself in check
        return None
    b = ch.Board(fen(white, "-"))
    if not np.array_equal(ch.encode_board(b).view(np.uint32).reshape(19, 8, 8), bits):        # e.g. rights the position cannot have
        return None
    ep = 255
    if mask is not None:
        up, fifth = (8, 4) if white else (-8, 3)
        for s in sorted(s for s, k in board.items() if k == (0 if white else 6) and (s >> 3) == fifth):
            for df in (-1, 1):
                t = s + up + df
                if not 0 <= (s & 7) + df < 8 or t in board or board.get(t - up) != (6 if white else 0) or ep != 255:
                    continue
                # the policy column of a one-step diagonal move: 73 per from-square, 7 per direction, directions in the
                # order N S E W NE NW SE SW (encoding.py:80-150)
                ray = {(1, 1): 4, (1, -1): 5, (-1, 1): 6, (-1, -1): 7}[(1 if white else -1, df)]
                if mask[s * 73 + ray * 7]:
                    ep = t
        if ep != 255:
            b = ch.Board(fen(white, ch.square_name(ep)))
    men = np.zeros(12, np.uint64)
    for s, k in board.items():
        men[k] |= np.uint64(1) << np.uint64(s)
    at_home = [(4, 5, 7, 3), (4, 5, 0, 3), (60, 11, 63, 9), (60, 11, 56, 9)]          # (king square, king, rook square, rook) per right
    from_men = sum(1 << i for i, (ks, k, rs, r) in enumerate(at_home) if board.get(ks) == k and board.get(rs) == r)
    return dict(men=men, turn=int(white), castling=castling, castling_from_men=from_men, ep=ep, halfmove=half, fullmove=full, fen=b.fen(),
                legal=np.flatnonzero(np.asarray(ch.get_legal_actions(b))).astype(np.uint16))


def pack_row(planes, pi, mask, mut=Mutations()):
    """One row -> dict(row_kind, mask_kind, pos: the 104 bytes, pi_idx, pi_val, mask_idx); a RAW row has empty entries"""
    pos = np.zeros(1, np.dtype([("men", "<u8", (12,)), ("f", "u1", (8,))]))
    p = position_of(planes, mask)
    binary = mask is None or bool((mask <= 1).all())
    none = np.zeros(0, np.uint16)
    if p is None or not binary:
        pos["f"][0, 5:7] = RAW, (MASK_NONE if mask is None else MASK_LIST)
        return dict(row_kind=RAW, mask_kind=int(pos["f"][0, 6]), pos=pos.view(np.uint8).reshape(104), pi_idx=none,
                    pi_val=np.zeros(0, np.float32), mask_idx=none)
    cols = np.flatnonzero(mask) if mask is not None else None
    same = mask is not None and np.array_equal(cols, p["legal"])
    mask_kind = MASK_NONE if mask is None else MASK_LEGAL if (same or mut.legal_on_mismatch) else MASK_LIST
    castling = p["castling_from_men"] if mut.castling_from_men else p["castling"]
    pos["men"][0] = p["men"]
    pos["f"][0] = (p["turn"], castling, 255 if mut.drop_ep else p["ep"], p["halfmove"], p["fullmove"], PACKED, mask_kind, 0)
    entries = np.flatnonzero(pi != 0.0) if mut.entry_by_value else np.flatnonzero(pi.view(np.uint32))
    return dict(row_kind=PACKED, mask_kind=mask_kind, pos=pos.view(np.uint8).reshape(104), pi_idx=entries.astype(np.uint16),
                pi_val=pi[entries].copy(), mask_idx=cols.astype(np.uint16) if mask_kind == MASK_LIST else none)


def fen_of(pos_bytes):
    """The FEN of a PACKED row's 104 bytes"""
    men, f = pos_bytes[:96].view("<u8"), pos_bytes[96:]
    board = {s: k for k in range(12) for s in range(64) if int(men[k]) >> s & 1}
    rows = []
    for r in range(7, -1, -1):
        row, gap = "", 0
        for file in range(8):
            k = board.get(r * 8 + file)
            if k is None:
                gap += 1
            else:
                row, gap = row + (str(gap) if gap else "") + PIECES[k], 0
        rows.append(row + (str(gap) if gap else ""))
    rights = "".join(c for i, c in enumerate("KQkq") if int(f[1]) >> i & 1) or "-"
    ep = "-" if f[2] == 255 else ch.square_name(int(f[2]))
    return f"{'/'.join(rows)} {'w' if f[0] else 'b'} {rights} {ep} {int(f[3])} {int(f[4])}"


def unpack_row(row, has_mask):
    """(planes, pi, mask or None) of a PACKED row of pack_row"""
    b = ch.Board(fen_of(row["pos"]))
    pi = np.zeros(COLS, np.float32)
    pi[row["pi_idx"]] = row["pi_val"]
    mask = None
    if has_mask:
        mask = np.zeros(COLS, np.uint8)
        if row["mask_kind"] == MASK_LIST:
            mask[row["mask_idx"]] = 1
        else:
            mask[:] = np.asarray(ch.get_legal_actions(b)).astype(np.uint8)
    return ch.encode_board(b).astype(np.float32), pi, mask


def pack_rows(s, pi, mask=None, mut=Mutations()):
    """Rows -> the arrays of m0_rowpack_arrays as a dict (z is carried as it is and left out)"""
    s, pi = np.ascontiguousarray(s, np.float32), np.ascontiguousarray(pi, np.float32)
    rows = [pack_row(s[i], pi[i], None if mask is None else mask[i], mut) for i in range(len(s))]
    raw = [i for i, r in enumerate(rows) if r["row_kind"] == RAW]
    off = lambda key: np.concatenate([[0], np.cumsum([len(r[key]) for r in rows])]).astype(np.int64)
    cat = lambda key, dtype: np.concatenate([r[key] for r in rows]).astype(dtype) if rows else np.zeros(0, dtype)
    return dict(pos=np.stack([r["pos"] for r in rows]), pi_off=off("pi_idx"), pi_idx=cat("pi_idx", np.uint16),
                pi_val=cat("pi_val", np.float32), mask_off=off("mask_idx"), mask_idx=cat("mask_idx", np.uint16),
                raw_planes=np.asarray(s)[raw].reshape(len(raw), 19, 8, 8), raw_pi=np.asarray(pi)[raw].reshape(len(raw), COLS),
                raw_mask=None if mask is None else np.asarray(mask)[raw].reshape(len(raw), COLS), rows=rows)
