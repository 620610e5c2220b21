// Input planes -> position: the inverse of encode_planes_f32 / plane_consts (chess_core.h), for stored training rows
// (s f32 [19][8][8], optionally the row's legal_mask u8 [4672]).  Shared by decode_planes_kernel (position_kernels.hip), which
// gathers the planes with wave ballots, and the host, which gathers them with loops (decode_planes_host below).
//
// What the planes hold: the men (0..11), the side to move (12), the CLEANED castling rights (13..16), min(halfmove, 99) / 99
// and min(fullmove, 199) / 199 as float32 of a double quotient (17, 18).  What they do not hold:
//   en passant   no plane.  With the row's mask: a pawn of the side to move on its fifth rank whose mask bit for the one-step
//                diagonal move points to an EMPTY square on the sixth rank with an enemy pawn directly behind it -- that square
//                is the en-passant square.  Without a mask ep stays none.  ep is therefore set only when a capture is legal
//                (make_move sets it after every double push): the same legal moves, planes and tkey, which reads has_legal_ep.
//   history      a search from planes sees no repetition with earlier positions.
//   clocks       a counter plane of exactly 1.0 means the cap OR MORE (flags below).
#pragma once
#include <string.h>
#include "../../include/m0_engine.h"
#include "chess_core.h"

namespace m0 {

// One row's planes as gathered: the twelve piece planes as bitboards in Pos order (a1 = bit 0), whether any piece-plane
// value was something else than exactly 0.0f / 1.0f, the seven constant planes' first values and whether any of them varies
// over the board.
struct PlaneBits {
    uint64_t pc[12];
    float c7[7];
    bool bad_piece_value;
    bool not_uniform;
};

M0_HD uint32_t f32_bits(float x) {
    uint32_t u;
#if defined(__HIP_DEVICE_COMPILE__)
    u = __float_as_uint(x);
#else
    memcpy(&u, &x, 4);
#endif
    return u;
}

// counter plane value -> k with x == float(double(k) / cap) bit for bit, or -1
M0_HD int counter_from_plane(float x, int cap) {
    if (!(x >= 0.f && x <= 1.f)) return -1;                   // NaN, negative, above the cap
    const int k = (int)((double)x * (double)cap + 0.5);        // round(x * cap): x >= 0
    if (k < 0 || k > cap) return -1;
    return f32_bits((float)((double)k / (double)cap)) == f32_bits(x) ? k : -1;
}

// An upper bound of what gen_moves<false> / gen_pseudo_wave write for p: the move lists hold M0_MAX_MOVES entries, and planes
// are not bound to reachable positions (a board of queens passes every other test).
M0_HD int pseudo_moves_bound(const Pos& p) {
    const int us = p.turn;
    const uint64_t own = occ_of(p, us), theirs = occ_of(p, us ^ 1), o = own | theirs;
    int n = 2 + 2;                                             // castling, en passant
    uint64_t pcs = own & ~p.bb[PAWN];
    while (pcs) { const int s = lsb(pcs); pcs &= pcs - 1; n += popc(piece_targets(p, s, piece_type_at(p, s))); }
    const uint64_t pawns = p.bb[PAWN] & own, promo_rank = RANK_1 | RANK_8;
    uint64_t c = pawns;
    while (c) {
        const int s = lsb(c); c &= c - 1;
        const uint64_t t = pawn_att(s, us) & theirs;
        n += popc(t & ~promo_rank) + 4 * popc(t & promo_rank);
    }
    const uint64_t single = (us == WHITE ? pawns << 8 : pawns >> 8) & ~o;
    n += popc(single & ~promo_rank) + 4 * popc(single & promo_rank) + popc(single);   // every single push may double
    return n;
}

// The position of gathered planes: M0_DECODE_OK with p and flags (M0_DECODE_HALFMOVE_SATURATED / _FULLMOVE_SATURATED) set, or
// the first reason in the order of include/m0_engine.h with p untouched.  ep is none (ep_from_mask).
M0_HD int pos_from_plane_bits(const PlaneBits& b, Pos& p, int& flags) {
    if (b.bad_piece_value) return M0_DECODE_PIECE_VALUE;
    uint64_t w = 0, k = 0, clash = 0, bbs[6];
    for (int t = 0; t < 6; ++t) {
        clash |= (w | k) & b.pc[t]; w |= b.pc[t];
        clash |= (w | k) & b.pc[6 + t]; k |= b.pc[6 + t];
        bbs[t] = b.pc[t] | b.pc[6 + t];
    }
    if (clash) return M0_DECODE_SQUARE_CLASH;
    if (popc(b.pc[KING]) != 1 || popc(b.pc[6 + KING]) != 1) return M0_DECODE_KINGS;
    if (bbs[PAWN] & (RANK_1 | RANK_8)) return M0_DECODE_PAWN_RANK;
    if (b.not_uniform) return M0_DECODE_NOT_UNIFORM;
    int bits5 = 0;
    for (int i = 0; i < 5; ++i) {
        const uint32_t u = f32_bits(b.c7[i]);
        if (u != 0u && u != 0x3f800000u) return M0_DECODE_FLAG_VALUE;
        bits5 |= (u ? 1 : 0) << i;
    }
    Pos q;
    for (int t = 0; t < 6; ++t) q.bb[t] = bbs[t];
    q.occ[BLACK] = k; q.occ[WHITE] = w;
    q.turn = (uint8_t)((bits5 & 1) ? WHITE : BLACK);
    q.cr = (uint8_t)(bits5 >> 1);                              // plane order = CR_WK, CR_WQ, CR_BK, CR_BQ bit order
    q.ep = -1; q.pad = 0; q.halfmove = 0; q.fullmove = 0;
    if (clean_cr(q) != q.cr) return M0_DECODE_CASTLING;        // the planes hold cleaned rights
    const int hm = counter_from_plane(b.c7[5], 99), fm = counter_from_plane(b.c7[6], 199);
    if (hm < 0 || fm < 0) return M0_DECODE_COUNTER;
    q.halfmove = (uint16_t)hm; q.fullmove = (uint16_t)fm;
    if (attacked(q, king_sq(q, q.turn ^ 1), q.turn)) return M0_DECODE_OPPONENT_IN_CHECK;
    if (pseudo_moves_bound(q) > M0_MAX_MOVES) return M0_DECODE_TOO_MANY_MOVES;
    flags |= (hm == 99 ? M0_DECODE_HALFMOVE_SATURATED : 0) | (fm == 199 ? M0_DECODE_FULLMOVE_SATURATED : 0);
    p = q;
    return M0_DECODE_OK;
}

// The en-passant square that the row's mask shows (header comment), -1 when there is none.  Every mask index read is
// move_to_index of a one-step diagonal move from a fifth-rank square: inside [0, M0_POLICY_SIZE).
M0_HD int ep_from_mask(const Pos& p, const uint8_t* mask) {
    const int us = p.turn, up = us == WHITE ? 8 : -8;
    const uint64_t o = occ_all(p), enemy_pawns = p.bb[PAWN] & occ_of(p, us ^ 1);
    uint64_t c = p.bb[PAWN] & occ_of(p, us) & (us == WHITE ? (RANK_1 << 32) : (RANK_1 << 24));
    while (c) {
        const int s = lsb(c); c &= c - 1;
        for (int df = -1; df <= 1; df += 2) {
            const int f = (s & 7) + df;
            if (f < 0 || f > 7) continue;
            const int t = s + up + df;
            if ((o & bit(t)) || !(enemy_pawns & bit(t - up))) continue;
            const int idx = move_to_index(p, mk_move(s, t, 0));
            if (idx >= 0 && idx < M0_POLICY_SIZE && mask[idx]) return t;
        }
    }
    return -1;
}

// ---- host: the same decode with loops instead of ballots (tests/planes_shim; no device code) ----
// planes f32 [19][64] in tensor order (row 0 = rank 8), mask u8 [M0_POLICY_SIZE] or null.  Returns the status; p is valid
// (and nlegal set) for M0_DECODE_OK and M0_DECODE_MASK_MISMATCH, zeroed otherwise.
inline PlaneBits gather_planes_host(const float* planes) {
    PlaneBits b;
    b.bad_piece_value = false; b.not_uniform = false;
    for (int k = 0; k < 12; ++k) {
        uint64_t t = 0;                                        // tensor order: bit n = tensor square n
        for (int n = 0; n < 64; ++n) {
            const uint32_t u = f32_bits(planes[k * 64 + n]);
            if (u == 0x3f800000u) t |= 1ull << n;
            else if (u != 0u) b.bad_piece_value = true;
        }
        b.pc[k] = __builtin_bswap64(t);                        // rank 8 first -> a1 = bit 0
    }
    for (int k = 0; k < 7; ++k) {
        b.c7[k] = planes[(12 + k) * 64];
        for (int n = 1; n < 64; ++n) if (f32_bits(planes[(12 + k) * 64 + n]) != f32_bits(b.c7[k])) b.not_uniform = true;
    }
    return b;
}
inline int decode_planes_host(const float* planes, const uint8_t* mask, Pos& p, int& flags, int& nlegal) {
    flags = mask ? 0 : M0_DECODE_NO_MASK;
    nlegal = 0;
    memset(&p, 0, sizeof(Pos));
    const PlaneBits b = gather_planes_host(planes);
    Pos q;
    const int st = pos_from_plane_bits(b, q, flags);
    if (st != M0_DECODE_OK) return st;
    p = q;
    if (mask) {
        const int ep = ep_from_mask(p, mask);
        if (ep >= 0) { p.ep = (int8_t)ep; flags |= M0_DECODE_EP_FROM_MASK; }
    }
    Move mv[M0_MAX_MOVES];
    nlegal = gen_legal(p, mv);
    if (!mask) return M0_DECODE_OK;
    // the legal moves' indices are distinct: the masks are equal when every one is set and nothing else is
    int set = 0;
    for (int j = 0; j < M0_POLICY_SIZE; ++j) set += mask[j] ? 1 : 0;
    bool ok = set == nlegal;
    for (int i = 0; i < nlegal && ok; ++i) {
        const int idx = move_to_index(p, mv[i]);
        ok = idx >= 0 && idx < M0_POLICY_SIZE && mask[idx];
    }
    return ok ? M0_DECODE_OK : M0_DECODE_MASK_MISMATCH;
}

}  // namespace m0
