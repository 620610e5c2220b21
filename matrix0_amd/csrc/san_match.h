// Reading moves back in: one written move (a SAN token, a UCI string or a raw move) becomes a 32-bit PATTERN without looking at
// any position, and a pattern is matched against the legal moves of a position.  Header-only, built on chess_core.h and
// compiled three times: for the device (replay_kernels.hip, one wave per game), for the host C ABI (capi_replay.hip) and for
// the CPU test shim (tests/replay_shim).
//
// THE PATTERN (uint32_t)
//   bits  0- 5  destination square (a1 = 0 ... h8 = 63)
//   bits  6- 8  moving piece type (PAWN = 0 ... KING = 5); not compared by an exact pattern
//   bits  9-12  from-file + 1 (a = 1 ... h = 8), 0 = not given
//   bits 13-16  from-rank + 1 (rank 1 = 1 ... rank 8 = 8), 0 = not given
//   bits 17-19  promotion piece as in a Move (0 none, 1 N, 2 B, 3 R, 4 Q)
//   bits 20-21  kind: SAN_KIND_SAN, SAN_KIND_CASTLE_SHORT, SAN_KIND_CASTLE_LONG, SAN_KIND_EXACT
//   bit  31     valid; the pattern 0 matches no move (a token that did not parse ends its game as ILLEGAL)
//
// THE RULE (python-chess Board.parse_san, restated over the legal-move list)
//   SAN      a legal move matches when the piece on its from-square has the pattern's type, its destination is the pattern's,
//            its from-file and from-rank agree where the pattern gives them, and its promotion equals the pattern's (a given
//            piece, or none: "e8" never matches e7e8q).  A pawn token without a from-file carries its destination's file as the
//            from-file, so "e4" never matches a capture.  The capture mark and the check suffix were dropped by the parser and
//            are not compared.  The king's two-file move is written O-O / O-O-O only: "Kg1" does not match castling.
//   CASTLE   the king's two-file move toward the g-file (short) or the c-file (long).
//   EXACT    from-square (file and rank both given), destination and promotion agree; the piece type is not looked at.
//   Exactly one matching move is the answer; none is SAN_ILLEGAL, more than one SAN_AMBIGUOUS.  An over-specified token ("Ngf3"
//   with one knight able to go there) resolves, as it does in python-chess.
#pragma once
#include "chess_core.h"

namespace m0 {

enum { SAN_KIND_SAN = 0, SAN_KIND_CASTLE_SHORT = 1, SAN_KIND_CASTLE_LONG = 2, SAN_KIND_EXACT = 3 };
enum { SAN_ILLEGAL = -1, SAN_AMBIGUOUS = -2 };      // san_match results below zero
constexpr uint32_t SAN_VALID = 1u << 31;

// How a replayed game ended (one per game) and what its final position is (bits).
enum { REPLAY_OK = 0, REPLAY_ILLEGAL = 1, REPLAY_AMBIGUOUS = 2, REPLAY_TOO_LONG = 3 };
enum { REPLAY_END_CHECKMATE = 1, REPLAY_END_STALEMATE = 2, REPLAY_END_INSUFFICIENT = 4, REPLAY_END_WHITE_TO_MOVE = 8 };

M0_HD uint32_t san_pack(int kind, int type, int from_file, int from_rank, int to, int promo) {
    return SAN_VALID | (uint32_t)to | ((uint32_t)type << 6) | ((uint32_t)(from_file + 1) << 9) |
           ((uint32_t)(from_rank + 1) << 13) | ((uint32_t)promo << 17) | ((uint32_t)kind << 20);
}
M0_HD int san_to(uint32_t pat) { return (int)(pat & 63u); }
M0_HD int san_type(uint32_t pat) { return (int)((pat >> 6) & 7u); }
M0_HD int san_from_file(uint32_t pat) { return (int)((pat >> 9) & 15u) - 1; }     // -1 = not given
M0_HD int san_from_rank(uint32_t pat) { return (int)((pat >> 13) & 15u) - 1; }    // -1 = not given
M0_HD int san_promo(uint32_t pat) { return (int)((pat >> 17) & 7u); }
M0_HD int san_kind(uint32_t pat) { return (int)((pat >> 20) & 3u); }

// The pattern of an exact move (an engine record's `played`, a UCI list).
M0_HD uint32_t san_exact_pattern(Move m) {
    return san_pack(SAN_KIND_EXACT, 0, mv_from(m) & 7, mv_from(m) >> 3, mv_to(m), mv_promo(m));
}

// Does the legal move m of p fit the pattern?
M0_HD bool san_move_matches(const Pos& p, Move m, uint32_t pat) {
    if (!(pat & SAN_VALID)) return false;
    const int from = mv_from(m), to = mv_to(m);
    const int kind = san_kind(pat);
    const int type = piece_type_at(p, from);
    const int df = (to & 7) - (from & 7);
    if (kind == SAN_KIND_CASTLE_SHORT) return type == KING && df == 2;
    if (kind == SAN_KIND_CASTLE_LONG) return type == KING && df == -2;
    if (to != san_to(pat) || mv_promo(m) != san_promo(pat)) return false;
    const int ff = san_from_file(pat), fr = san_from_rank(pat);
    if (ff >= 0 && (from & 7) != ff) return false;
    if (fr >= 0 && (from >> 3) != fr) return false;
    if (kind == SAN_KIND_EXACT) return true;
    if (type != san_type(pat)) return false;
    return !(type == KING && (df == 2 || df == -2));
}

// The one legal move of p (moves[0..n) = its legal moves) that fits the pattern, or SAN_ILLEGAL / SAN_AMBIGUOUS.
M0_HD int san_match(const Pos& p, const Move* moves, int n, uint32_t pat) {
    int hit = SAN_ILLEGAL;
    for (int i = 0; i < n; ++i) {
        if (!san_move_matches(p, moves[i], pat)) continue;
        if (hit >= 0) return SAN_AMBIGUOUS;
        hit = (int)moves[i];
    }
    return hit;
}

// End flags of a position with nlegal legal moves.
M0_HD int replay_end_flags(const Pos& p, int nlegal) {
    const bool chk = in_check(p);
    return (nlegal == 0 && chk ? REPLAY_END_CHECKMATE : 0) | (nlegal == 0 && !chk ? REPLAY_END_STALEMATE : 0) |
           (is_insufficient(p) ? REPLAY_END_INSUFFICIENT : 0) | (p.turn == WHITE ? REPLAY_END_WHITE_TO_MOVE : 0);
}

// ---- host only: text -> pattern ----
// One SAN token -> pattern; false for anything python-chess's SAN reader would not take as a move of the board: its grammar is
//   [NBRQK]? [a-h]? [1-8]? [-x]? [a-h][1-8] (=?[NBRQnbrq])? [+#]?      or      O-O / O-O-O / 0-0 / 0-0-0  [+#]?
// after trailing '!' / '?' annotations are dropped.  The null moves "--" and "Z0" are refused with everything else.
inline bool san_parse_token(const char* tok, uint32_t* pattern) {
    *pattern = 0;
    if (!tok) return false;
    int n = 0;
    while (tok[n]) ++n;
    while (n > 0 && (tok[n - 1] == '!' || tok[n - 1] == '?')) --n;
    if (n > 0 && (tok[n - 1] == '+' || tok[n - 1] == '#')) --n;
    auto is = [&](const char* s) { int k = 0; while (s[k]) ++k; if (k != n) return false; for (int i = 0; i < n; ++i) if (tok[i] != s[i]) return false; return true; };
    if (is("O-O") || is("0-0")) { *pattern = san_pack(SAN_KIND_CASTLE_SHORT, KING, -1, -1, 0, 0); return true; }
    if (is("O-O-O") || is("0-0-0")) { *pattern = san_pack(SAN_KIND_CASTLE_LONG, KING, -1, -1, 0, 0); return true; }
    auto file_of = [](char c) { return c >= 'a' && c <= 'h' ? c - 'a' : -1; };
    auto rank_of = [](char c) { return c >= '1' && c <= '8' ? c - '1' : -1; };
    auto promo_of = [](char c) {
        switch (c) { case 'N': case 'n': return 1; case 'B': case 'b': return 2; case 'R': case 'r': return 3; case 'Q': case 'q': return 4; default: return 0; }
    };
    // from the back: promotion, destination; from the front: piece letter; what is left is [a-h]?[1-8]?[-x]?
    int promo = 0;
    if (n >= 3 && promo_of(tok[n - 1]) && rank_of(tok[n - 2]) >= 0) {
        promo = promo_of(tok[n - 1]);
        n -= 1;
    } else if (n >= 4 && promo_of(tok[n - 1]) && tok[n - 2] == '=') {
        promo = promo_of(tok[n - 1]);
        n -= 2;
    }
    if (n < 2) return false;
    const int tf = file_of(tok[n - 2]), tr = rank_of(tok[n - 1]);
    if (tf < 0 || tr < 0) return false;
    n -= 2;
    int i = 0, type = PAWN;
    if (i < n) {
        switch (tok[i]) {
            case 'N': type = KNIGHT; ++i; break; case 'B': type = BISHOP; ++i; break; case 'R': type = ROOK; ++i; break;
            case 'Q': type = QUEEN; ++i; break; case 'K': type = KING; ++i; break; default: break;
        }
    }
    int ff = -1, fr = -1;
    if (i < n && file_of(tok[i]) >= 0) ff = file_of(tok[i++]);
    if (i < n && rank_of(tok[i]) >= 0) fr = rank_of(tok[i++]);
    if (i < n && (tok[i] == 'x' || tok[i] == '-')) ++i;
    if (i != n) return false;
    if (type == PAWN && ff < 0) ff = tf;                 // python-chess: no pawn capture without the from-file
    *pattern = san_pack(SAN_KIND_SAN, type, ff, fr, tr * 8 + tf, promo);
    return true;
}

// A UCI string ("e2e4", "e7e8q") -> exact pattern; false for anything else ("0000" included).
inline bool san_parse_uci(const char* uci, uint32_t* pattern) {
    *pattern = 0;
    if (!uci) return false;
    int n = 0;
    while (uci[n]) ++n;
    if (n != 4 && n != 5) return false;
    for (int i = 0; i < 4; i += 2)
        if (uci[i] < 'a' || uci[i] > 'h' || uci[i + 1] < '1' || uci[i + 1] > '8') return false;
    int promo = 0;
    if (n == 5) {
        switch (uci[4]) { case 'n': promo = 1; break; case 'b': promo = 2; break; case 'r': promo = 3; break; case 'q': promo = 4; break; default: return false; }
    }
    *pattern = san_exact_pattern(mk_move((uci[0] - 'a') + 8 * (uci[1] - '1'), (uci[2] - 'a') + 8 * (uci[3] - '1'), promo));
    return true;
}

// A raw move value from | to<<6 | promo<<12 -> exact pattern; false when bits outside the move are set or promo > 4.
inline bool san_parse_raw(uint32_t raw, uint32_t* pattern) {
    *pattern = 0;
    if (raw > 0x7FFFu || ((raw >> 12) & 7u) > 4u) return false;
    *pattern = san_exact_pattern((Move)raw);
    return true;
}

}  // namespace m0
