// Board.fen() text of a position, shared by the C-ABI units that write FENs (m0_fen_after, m0_decode_planes).  Host only.
#pragma once
#include <string>
#include "chess_core.h"

namespace m0 {

// Board.fen() of python-chess (en_passant="legal": the ep square only when an en-passant capture is legal; cleaned castling rights)
inline std::string fen_of(const Pos& p) {
    std::string s;
    for (int r = 7; r >= 0; --r) {
        int e = 0;
        for (int f = 0; f < 8; ++f) {
            const int sq = r * 8 + f;
            const uint64_t b = bit(sq);
            if (!((p.occ[0] | p.occ[1]) & b)) { ++e; continue; }
            if (e) { s += (char)('0' + e); e = 0; }
            const int t = piece_type_at(p, sq);
            s += ((p.occ[WHITE] & b) ? "PNBRQK" : "pnbrqk")[t];
        }
        if (e) s += (char)('0' + e);
        if (r) s += '/';
    }
    s += p.turn == WHITE ? " w " : " b ";
    const int cr = clean_cr(p);
    std::string c;
    if (cr & CR_WK) c += 'K';
    if (cr & CR_WQ) c += 'Q';
    if (cr & CR_BK) c += 'k';
    if (cr & CR_BQ) c += 'q';
    s += c.empty() ? "-" : c;
    s += ' ';
    if (p.ep >= 0 && has_legal_ep(p)) { s += (char)('a' + (p.ep & 7)); s += (char)('1' + (p.ep >> 3)); }
    else s += '-';
    s += ' ' + std::to_string(p.halfmove) + ' ' + std::to_string(p.fullmove);
    return s;
}

}  // namespace m0
