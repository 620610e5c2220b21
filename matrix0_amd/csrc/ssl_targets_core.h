// The reference's SSL target maps for ONE square (azchess/ssl_algorithms.py:51-143, 256-557), as a function of the board's 64
// pieces and the side to move.  Plain C++ without intrinsics, host and device: ssl_targets_kernel (position_kernels.hip) runs it on
// the pieces of a Pos, ssl_targets_planes_kernel and ssl_score_kernel on the pieces read back from stored planes, and
// tests/ssl_score_shim under g++.
//
// All geometry is in tensor space (square = row * 8 + column, row 0 = rank 8) exactly as the reference computes it, quirks
// included (SURVEY B-5): white pawns attack toward higher row index; the reference's pin map is identically zero (it ANDs a map
// that is non-zero only on the candidate square with one non-zero only on the next square).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define M0_SSL_HD __host__ __device__ inline
#else
#define M0_SSL_HD inline
#endif

namespace m0ssl {

constexpr int TARGET_CH = 17;          // a row of target maps: piece one-hot (13), threat, pin, fork, control
constexpr int PIECE_CH = 13;
constexpr int PLANES_READ = 13;        // of a row of stored planes: the 12 piece planes and the side to move

struct SquareTargets {
    int piece;          // plane index 0..11 (white P..K, black P..K) or -1 on an empty square
    bool threat, fork;  // (pin is always 0)
    int control;        // sign(white attackers - black attackers)
};

// `board(sq)`: the piece on tensor square sq in 0..63, as SquareTargets::piece
template <class Board>
M0_SSL_HD SquareTargets square_targets(const Board& board, int sq, bool stm_white) {
    const int r = sq >> 3, c = sq & 7;
    auto at = [&](int rr, int cc) -> int { return ((unsigned)rr < 8u && (unsigned)cc < 8u) ? (int)board(rr * 8 + cc) : -2; };
    const int KN[8][2] = {{-2, -1}, {-2, 1}, {-1, -2}, {-1, 2}, {1, -2}, {1, 2}, {2, -1}, {2, 1}};
    const int KG[8][2] = {{-1, -1}, {-1, 0}, {-1, 1}, {0, -1}, {0, 1}, {1, -1}, {1, 0}, {1, 1}};
    int wa = 0, ba = 0;
    // pawns: white pawn at (r0,c0) attacks (r0+1,c0+-1); black pawn attacks (r0-1,c0+-1)
    for (int dc = -1; dc <= 1; dc += 2) {
        if (at(r - 1, c + dc) == 0) ++wa;
        if (at(r + 1, c + dc) == 6) ++ba;
    }
    for (int k = 0; k < 8; ++k) {
        int q = at(r + KN[k][0], c + KN[k][1]);
        if (q == 1) ++wa; else if (q == 7) ++ba;
        q = at(r + KG[k][0], c + KG[k][1]);
        if (q == 5) ++wa; else if (q == 11) ++ba;
    }
    const int me = board(sq);
    const bool own_tactical = me >= 0 && ((stm_white && me >= 1 && me <= 5) || (!stm_white && me >= 7 && me <= 11));
    const int mytype = me >= 0 ? me % 6 : -1;          // 0 P,1 N,2 B,3 R,4 Q,5 K
    int forks = 0;
    if (own_tactical && (mytype == 1 || mytype == 5)) {
        for (int k = 0; k < 8; ++k) {
            const int q = mytype == 1 ? at(r + KN[k][0], c + KN[k][1]) : at(r + KG[k][0], c + KG[k][1]);
            if (q >= 0 && ((q < 6) != stm_white)) ++forks;
        }
    }
    for (int k = 0; k < 8; ++k) {                       // the 8 ray directions (KG is also the ray set)
        const int dr = KG[k][0], dc = KG[k][1];
        const bool diag = dr != 0 && dc != 0;
        int rr = r + dr, cc = c + dc, q = -1;
        while ((unsigned)rr < 8u && (unsigned)cc < 8u) {
            q = board(rr * 8 + cc);
            if (q >= 0) break;
            rr += dr; cc += dc;
        }
        if (q < 0) continue;
        const int t = q % 6;
        // the first piece along the ray attacks this square if it slides along the ray
        if (t == 4 || (diag && t == 2) || (!diag && t == 3)) { if (q < 6) ++wa; else ++ba; }
        // and this square's own slider attacks that first piece if it is an enemy
        if (own_tactical && (mytype == 4 || (diag && mytype == 2) || (!diag && mytype == 3)) && ((q < 6) != stm_white)) ++forks;
    }
    SquareTargets t;
    t.piece = me;
    t.threat = (stm_white ? ba : wa) > 0;
    t.fork = own_tactical && forks >= 2;
    t.control = wa > ba ? 1 : (wa < ba ? -1 : 0);
    return t;
}

// the square's 17 values of a row of target maps [17][64]
M0_SSL_HD void store_square(const SquareTargets& t, float* row, int sq) {
    for (int k = 0; k < 12; ++k) row[k * 64 + sq] = t.piece == k ? 1.f : 0.f;
    row[12 * 64 + sq] = t.piece < 0 ? 1.f : 0.f;
    row[13 * 64 + sq] = t.threat ? 1.f : 0.f;
    row[14 * 64 + sq] = 0.f;
    row[15 * 64 + sq] = t.fork ? 1.f : 0.f;
    row[16 * 64 + sq] = (float)t.control;
}

// ---- the board of a row of stored planes f32 [19][64] (encode_board, encoding.py:11-46: planes 0-11 the pieces, 12 the side
// to move).  A row is usable when every value of planes 0-11 is 0 or 1, no square has two pieces, and plane 12 is one value over
// the board, 0 or 1.  Nothing else enters the targets.

// the piece the planes put on `sq` (-1: none); *bad when a value there is neither 0 nor 1 or two planes claim the square
M0_SSL_HD int plane_piece(const float* planes_row, int sq, bool* bad) {
    int piece = -1, n = 0;
    bool off = false;
    for (int k = 0; k < 12; ++k) {
        const float v = planes_row[k * 64 + sq];
        if (v == 1.f) { piece = k; ++n; }
        else if (!(v == 0.f)) off = true;            // also NaN
    }
    *bad = off || n > 1;
    return n == 1 ? piece : -1;
}

// plane 12 at one square against its value at square 0
M0_SSL_HD bool side_bad(float here, float first) { return !(here == first) || !(first == 0.f || first == 1.f); }

// 64 pieces in four 64-bit words: bit sq of word j is bit j of (piece + 1).  A wave fills it with four ballots, the host square
// by square; every lane then reads any square without shared memory.
struct Board4 {
    uint64_t w[4] = {0, 0, 0, 0};
    M0_SSL_HD void set(int sq, int piece) {
        const unsigned code = (unsigned)(piece + 1);
        for (int j = 0; j < 4; ++j) w[j] |= (uint64_t)((code >> j) & 1u) << sq;
    }
    M0_SSL_HD int operator()(int sq) const {
        unsigned code = 0;
        for (int j = 0; j < 4; ++j) code |= (unsigned)((w[j] >> sq) & 1ull) << j;
        return (int)code - 1;
    }
};

}  // namespace m0ssl
