// TEST INFRASTRUCTURE: host (g++) build of matrix0_amd/csrc/san_match.h with a scalar replay over gen_legal, so that the token
// parser, the matching rule and the per-ply outputs of the replay kernel can be checked on the CPU and serve as the expected
// values of the GPU tests.  Not part of libm0engine.so.
#include <string.h>
#include "../../matrix0_amd/csrc/san_match.h"
using namespace m0;

extern "C" {

int rs_san_pattern(const char* token, uint32_t* pattern) { return san_parse_token(token, pattern) ? 0 : -1; }
int rs_uci_pattern(const char* uci, uint32_t* pattern) { return san_parse_uci(uci, pattern) ? 0 : -1; }
int rs_raw_pattern(uint32_t raw, uint32_t* pattern) { return san_parse_raw(raw, pattern) ? 0 : -1; }

// fields of a pattern: out[0..6] = kind, piece type, from-file (-1 none), from-rank (-1 none), destination, promotion, valid
void rs_pattern_fields(uint32_t pat, int32_t* out) {
    out[0] = san_kind(pat); out[1] = san_type(pat); out[2] = san_from_file(pat); out[3] = san_from_rank(pat);
    out[4] = san_to(pat); out[5] = san_promo(pat); out[6] = (pat & SAN_VALID) ? 1 : 0;
}

// One game, as replay_games_kernel defines it: rows [0, *plies) of the per-ply outputs are written (position BEFORE the move),
// the others are left alone.  planes (f32 [n][19][64]) may be null.  Returns -1 for a bad FEN (null = initial position).
int rs_replay(const char* fen, const uint32_t* patterns, int n, int max_plies, uint16_t* moves, int32_t* policy_idx,
              int32_t* nlegal, int8_t* turn, float* planes, int32_t* plies, int32_t* status, int32_t* end_flags) {
    Pos p;
    if (parse_fen(fen ? fen : "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1", p)) return -1;
    Move mv[M0_MAX_MOVES];
    const int lim = n < max_plies ? n : max_plies;
    int st = REPLAY_OK, ply = 0;
    int k = gen_legal(p, mv);
    while (ply < lim) {
        const int hit = san_match(p, mv, k, patterns[ply]);
        if (hit < 0) { st = hit == SAN_AMBIGUOUS ? REPLAY_AMBIGUOUS : REPLAY_ILLEGAL; break; }
        moves[ply] = (Move)hit;
        policy_idx[ply] = move_to_index(p, (Move)hit);
        nlegal[ply] = k;
        turn[ply] = (int8_t)p.turn;
        if (planes) encode_planes_f32(p, planes + (size_t)ply * 19 * 64);
        make_move(p, (Move)hit);
        ++ply;
        k = gen_legal(p, mv);
    }
    if (st == REPLAY_OK && n > max_plies) st = REPLAY_TOO_LONG;
    *plies = ply; *status = st; *end_flags = replay_end_flags(p, k);
    return 0;
}
}
