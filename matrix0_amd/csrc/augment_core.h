// The trainer's flip and rotate augmentations of a stored row, defined once for the host and the device (include/m0_augment.h;
// the reference: azchess/training/train.py:280-305 with the permutations of azchess/encoding.py:310-386).
//
// A row's policy is [rank][file][73] (4672 columns, square = rank * 8 + file), its planes [P][rank][file].  A kind is a map of the
// squares and a permutation of the 73 move-type channels:
//   s'[p][sq] = s[p][map(sq)]      pi'[sq][c] = pi[map(sq)][perm[c]]      legal_mask' as pi'
// The 73 channels: 8 ray directions N, S, E, W, NE, NW, SE, SW of 7 steps each (channel = direction * 7 + step - 1), 8 knight jumps
// (56-63), and 3 under-promotion pieces of 3 directions each (64 + piece * 3 + {0 forward, 1 and 2 the two captures}).
//   HFLIP   file -> 7 - file; rays E<->W, NE<->NW, SE<->SW per step; knights in the pairs (56,57) (58,59) (60,61) (62,63); the two
//           capture directions of every under-promotion block swapped, forward kept.
//   ROT180  rank -> 7 - rank and file -> 7 - file; rays N<->S, E<->W, NE<->SW, NW<->SE per step; knights in the pairs (56,63) (57,62)
//           (58,61) (59,60); under-promotions as under HFLIP.
// Both maps and both permutations are involutions: a kind applied twice gives the row back.
//
// This is what the trainer does, reproduced and not corrected.  ROT180 without a swap of the colours is not a symmetry of chess:
// white pawns of the rotated planes stand on their seventh rank and move backwards, and the side-to-move, castling and counter
// planes stay as they were.  HFLIP is a symmetry of chess only for positions without castling rights: the castling planes are not
// exchanged between the king's and the queen's side, and a mirrored castling move is no castling move.
#pragma once
#include <stdint.h>
#include "../../include/m0_engine.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define M0_AUG_HD __host__ __device__
#else
#define M0_AUG_HD
#endif

namespace m0aug {

constexpr int CHANNELS = 73;
constexpr int SQUARES = 64;
constexpr int COLS = CHANNELS * SQUARES;        // 4672
constexpr int KINDS = 3;
constexpr int RAY_STEPS = 7, KNIGHT0 = 56, UNDER0 = 64;

// the ray direction that direction d (N S E W NE NW SE SW) is read from
constexpr uint8_t RAY_FROM[KINDS][8] = {{0, 1, 2, 3, 4, 5, 6, 7}, {0, 1, 3, 2, 5, 4, 7, 6}, {1, 0, 3, 2, 7, 6, 5, 4}};

struct Perm {
    uint8_t at[CHANNELS];
};

constexpr Perm make_perm(int kind) {
    Perm p{};
    for (int c = 0; c < CHANNELS; ++c) {
        int from = c;
        if (c < KNIGHT0) from = RAY_FROM[kind][c / RAY_STEPS] * RAY_STEPS + c % RAY_STEPS;
        else if (c < UNDER0) from = kind == M0_AUG_HFLIP ? KNIGHT0 + ((c - KNIGHT0) ^ 1) : kind == M0_AUG_ROT180 ? KNIGHT0 + 7 - (c - KNIGHT0) : c;
        else if (kind != M0_AUG_NONE) {
            const int dir = (c - UNDER0) % 3;
            from = c - dir + (dir == 0 ? 0 : 3 - dir);
        }
        p.at[c] = (uint8_t)from;
    }
    return p;
}

// perm_k of the header, for k = M0_AUG_NONE (the identity), M0_AUG_HFLIP, M0_AUG_ROT180
constexpr Perm PERM[KINDS] = {make_perm(M0_AUG_NONE), make_perm(M0_AUG_HFLIP), make_perm(M0_AUG_ROT180)};
// map(sq) = sq ^ SQUARE_XOR[kind]: the files are the low three bits of a square, the ranks the high three
constexpr int SQUARE_XOR[KINDS] = {0, 7, 63};

M0_AUG_HD constexpr bool valid_kind(int kind) { return kind >= 0 && kind < KINDS; }
M0_AUG_HD constexpr int map_square(int kind, int sq) { return sq ^ (kind == M0_AUG_HFLIP ? 7 : kind == M0_AUG_ROT180 ? 63 : 0); }

// the column of pi (and of the mask) that output column `col` of a row of this kind is read from
M0_AUG_HD constexpr int source_column(int kind, int col) {
    const int sq = col / CHANNELS, c = col - sq * CHANNELS;
    int from = c;                                  // make_perm's rule for one channel, without building the table
    if (c < KNIGHT0) {
        const int d = c / RAY_STEPS;
        const int fd = kind == M0_AUG_HFLIP ? (d < 2 ? d : d ^ 1) : kind == M0_AUG_ROT180 ? (d < 4 ? d ^ 1 : 11 - d) : d;
        from = fd * RAY_STEPS + (c - d * RAY_STEPS);
    } else if (c < UNDER0) {
        from = kind == M0_AUG_HFLIP ? KNIGHT0 + ((c - KNIGHT0) ^ 1) : kind == M0_AUG_ROT180 ? KNIGHT0 + 7 - (c - KNIGHT0) : c;
    } else if (kind != M0_AUG_NONE) {
        const int dir = (c - UNDER0) % 3;
        from = c - dir + (dir == 0 ? 0 : 3 - dir);
    }
    return map_square(kind, sq) * CHANNELS + from;
}

// the two definitions above are one: every channel of every kind, on the first square and on one in the middle of the board
constexpr bool columns_agree() {
    for (int k = 0; k < KINDS; ++k)
        for (int sq = 0; sq < SQUARES; sq += 27)
            for (int c = 0; c < CHANNELS; ++c)
                if (source_column(k, sq * CHANNELS + c) != (sq ^ SQUARE_XOR[k]) * CHANNELS + PERM[k].at[c]) return false;
    return true;
}
static_assert(columns_agree(), "source_column and PERM disagree");

// One row on the host, as augment_rows_kernel moves it.  planes / planes_out [P][64], pi / pi_out [4672], mask / mask_out [4672] or
// both null; input and output do not overlap.  Values travel as their bits.
inline void augment_row(int kind, const uint32_t* planes, int P, const uint32_t* pi, const uint8_t* mask, uint32_t* planes_out,
                        uint32_t* pi_out, uint8_t* mask_out) {
    for (int p = 0; p < P; ++p)
        for (int sq = 0; sq < SQUARES; ++sq) planes_out[p * SQUARES + sq] = planes[p * SQUARES + map_square(kind, sq)];
    for (int col = 0; col < COLS; ++col) {
        const int from = source_column(kind, col);
        pi_out[col] = pi[from];
        if (mask) mask_out[col] = mask[from];
    }
}

}  // namespace m0aug
