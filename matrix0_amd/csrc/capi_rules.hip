// extern "C" host functions that touch neither an engine nor the GPU (include/m0_engine.h): the sampling and playout rules,
// the rules probe, SAN and FEN text.
#include <hip/hip_runtime.h>      // no hip* call here: the __device__ half of chess_core.h needs its intrinsics when built as HIP
#include <stdlib.h>
#include <string.h>
#include <string>
#include "../../include/m0_engine.h"
#include "capi_common.h"
#include "chess_core.h"
#include "fen_text.h"
#include "host_rules.h"

using namespace m0;

// Standard algebraic notation of a legal move (python-chess Board.san semantics: piece letter, minimal
// disambiguation by file, then rank, then both; 'x'; '=Q'; O-O / O-O-O; '+' / '#') -- PGN output of arena games
// (arena.py:281-303 writes them with chess.pgn).
static std::string san_of(const Pos& p, Move m, const Move* legal, int nlegal) {
    const int from = mv_from(m), to = mv_to(m), promo = mv_promo(m);
    const int pt = piece_type_at(p, from);
    std::string s;
    if (pt == KING && abs((to & 7) - (from & 7)) == 2) {
        s = (to & 7) > (from & 7) ? "O-O" : "O-O-O";
    } else {
        const bool capture = ((occ_of(p, p.turn ^ 1) >> to) & 1ull) || (pt == PAWN && (from & 7) != (to & 7));
        if (pt != PAWN) {
            s += "NBRQK"[pt - 1];
            bool any = false, same_file = false, same_rank = false;
            for (int i = 0; i < nlegal; ++i) {
                const Move o = legal[i];
                if (o == m || mv_to(o) != to || mv_from(o) == from || piece_type_at(p, mv_from(o)) != pt) continue;
                any = true;
                if ((mv_from(o) & 7) == (from & 7)) same_file = true;
                if ((mv_from(o) >> 3) == (from >> 3)) same_rank = true;
            }
            if (any) {
                if (!same_file) s += (char)('a' + (from & 7));
                else if (!same_rank) s += (char)('1' + (from >> 3));
                else { s += (char)('a' + (from & 7)); s += (char)('1' + (from >> 3)); }
            }
        } else if (capture) {
            s += (char)('a' + (from & 7));
        }
        if (capture) s += 'x';
        s += (char)('a' + (to & 7));
        s += (char)('1' + (to >> 3));
        if (promo) { s += '='; s += "NBRQ"[promo - 1]; }
    }
    Pos q = p;
    make_move(q, m);
    if (in_check(q)) s += any_legal(q) ? '+' : '#';
    return s;
}

// parses a UCI move and plays it on ln; false with "Illegal move: ..." set when it is not legal there
static bool play_uci(Line& ln, const char* uci) {
    Move legal[M0_MAX_MOVES];
    int n;
    if (ln.play_if_legal(uci ? parse_uci(uci) : (Move)0xFFFF, legal, n)) return true;
    m0_set_error(std::string("Illegal move: ") + (uci ? uci : "(null)"));
    return false;
}

extern "C" {

int m0_sample_move_index(const int32_t* visits, int n, double temperature, double u) {
    if (!visits || n <= 0) return -1;
    return sample_move_index(visits, n, temperature, u);
}
int m0_playout_cap(int sims, double frac, double u) { return playout_cap(sims, frac, u); }
double m0_temperature_for(int fullmove_number, double t_start, double t_end, int t_moves) {
    return temperature_for(fullmove_number, t_start, t_end, t_moves);
}
int m0_rules_probe(const m0_selfplay_cfg* cfg, const char* fen, const char* const* ucis, int n, int* flags, float* result) {
    if (!cfg || !fen || !flags) { m0_set_error("null argument"); return M0_ERR_INVALID; }
    Line ln;
    Pos& p = ln.pos;
    if (parse_fen(fen, p) != 0) { m0_set_error("bad FEN"); return M0_ERR_INVALID; }
    const RepWindow& w = ln.win;
    for (int i = 0; i < n; ++i)
        if (!play_uci(ln, ucis[i])) return M0_ERR_INVALID;
    DrawCfg dc = draw_cfg_from(*cfg);
    int f = 0;
    if (is_game_over(p, w, false)) f |= 1;
    if (is_game_over(p, w, true)) f |= 2;
    if (should_adjudicate_draw(p, w, ln.history, dc)) f |= 4;
    const bool anyl = any_legal(p), chk = in_check(p);
    if (!anyl && chk) f |= 8;
    if (!anyl && !chk) f |= 16;
    if (is_insufficient(p)) f |= 32;
    if (can_claim_fifty(p)) f |= 64;
    if (w.is_repetition(p, 3)) f |= 128;
    if (w.can_claim_threefold(p)) f |= 256;
    if (w.is_repetition(p, 5)) f |= 512;
    if (p.halfmove >= 150 && anyl) f |= 1024;
    *flags = f;
    if (result) *result = game_result(p);
    return M0_OK;
}

int m0_arena_choose_move(const int32_t* visits, int n, double temp, int ply, int temp_plies, double u) {
    if (!visits || n <= 0) { m0_set_error("empty visit list"); return M0_ERR_INVALID; }
    return arena_choose_move(visits, n, temp, ply, temp_plies, u);
}

int m0_san_legal_fen(const char* fen, uint16_t* moves, char* san, int* nlegal) {
    if (!fen || !moves || !san || !nlegal) { m0_set_error("null argument"); return M0_ERR_INVALID; }
    Pos p;
    if (parse_fen(fen, p) != 0) { m0_set_error("bad FEN"); return M0_ERR_INVALID; }
    Move mv[M0_MAX_MOVES];
    const int k = gen_legal(p, mv);
    for (int i = 0; i < k; ++i) {
        moves[i] = mv[i];
        const std::string t = san_of(p, mv[i], mv, k);
        memset(san + 8 * i, 0, 8);
        memcpy(san + 8 * i, t.c_str(), t.size() < 8 ? t.size() : 7);
    }
    *nlegal = k;
    return M0_OK;
}

int m0_fen_after(const char* fen, const char* const* ucis, int n, char* fen_out, int cap) {
    if (!fen || !fen_out || cap <= 0 || (n > 0 && !ucis)) { m0_set_error("null argument"); return M0_ERR_INVALID; }
    Line ln;
    if (parse_fen(fen, ln.pos) != 0) { m0_set_error("bad FEN"); return M0_ERR_INVALID; }
    for (int i = 0; i < n; ++i)
        if (!play_uci(ln, ucis[i])) return M0_ERR_INVALID;
    const std::string f = fen_of(ln.pos);
    if ((int)f.size() + 1 > cap) { m0_set_error("output buffer too small"); return M0_ERR_INVALID; }
    memcpy(fen_out, f.c_str(), f.size() + 1);
    return M0_OK;
}

int m0_san_game(const uint16_t* moves, int n, char* out, int cap) { return m0_san_game_fen(START_FEN, moves, n, out, cap); }

int m0_san_game_fen(const char* fen, const uint16_t* moves, int n, char* out, int cap) {
    if (!fen || (!moves && n > 0) || !out || cap <= 0) { m0_set_error("null argument"); return M0_ERR_INVALID; }
    Line ln;
    if (parse_fen(fen, ln.pos) != 0) { m0_set_error("bad FEN"); return M0_ERR_INVALID; }
    std::string text;
    for (int i = 0; i < n; ++i) {
        const Pos before = ln.pos;
        Move mv[M0_MAX_MOVES];
        int k;
        if (!ln.play_if_legal(moves[i], mv, k)) { m0_set_error("illegal move in game"); return M0_ERR_INVALID; }
        // the number in front of every White move and, as python-chess writes a line that Black opens, "12..." in front of
        // the first move
        if (before.turn == WHITE) text += std::to_string(before.fullmove) + ". ";
        else if (i == 0) text += std::to_string(before.fullmove) + "... ";
        text += san_of(before, moves[i], mv, k);
        text += ' ';
    }
    if ((int)text.size() + 1 > cap) { m0_set_error("output buffer too small"); return M0_ERR_INVALID; }
    memcpy(out, text.c_str(), text.size() + 1);
    return (int)text.size();
}

}  // extern "C"
