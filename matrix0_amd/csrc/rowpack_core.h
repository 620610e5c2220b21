// Per-row arithmetic of the packed training rows (include/m0_rowpack.h), host and device: rowpack_kernels.hip runs it one wave
// per row with a lane per 16-byte piece, capi_rowpack.hip runs it on the CPU with plain loops (m0_rowpack_*_host), and
// tests/rowpack_shim runs the kernels' lane split as a loop under g++.  Nothing here decodes or encodes planes: packing takes the
// position that planes_decode.h found, unpacking hands a position to the encoder of chess_core.h.
#pragma once
#include <stdint.h>
#include "../../include/m0_engine.h"
#include "chess_core.h"
#include "planes_decode.h"

namespace m0rowpack {

using m0::Pos;

constexpr int COLS = M0_POLICY_SIZE;
constexpr int LANES = 64;
constexpr int PLANE_FLOATS = M0_PLANES * 64;
// a row as 16-byte pieces; piece k * 64 + lane belongs to lane `lane` in sweep k
constexpr int PI_PIECES = COLS / 4;                                   // 1168: 19 sweeps, the last partial
constexpr int PI_SWEEPS = (PI_PIECES + LANES - 1) / LANES;
constexpr int MASK_PIECES = COLS / 16;                                // 292: 5 sweeps, the last partial
constexpr int MASK_SWEEPS = (MASK_PIECES + LANES - 1) / LANES;
constexpr int PLANE_PIECES = PLANE_FLOATS / 4;                        // 304
static_assert(COLS % 16 == 0 && PLANE_FLOATS % 4 == 0, "rows are moved in 16-byte pieces");
static_assert(sizeof(m0_rowpack_pos) == 104, "m0_rowpack_pos is 104 bytes: twelve bitboards and eight bytes");
static_assert(COLS <= 65536, "columns are stored as uint16");

// ---- kinds ----
// status: what the decode said of the row's planes (and mask); mask_binary: every mask byte is 0 or 1
M0_HD void row_kinds(int status, bool has_mask, bool mask_binary, int& row_kind, int& mask_kind) {
    const bool decoded = status == M0_DECODE_OK || status == M0_DECODE_MASK_MISMATCH;
    row_kind = decoded && (!has_mask || mask_binary) ? M0_ROWPACK_PACKED : M0_ROWPACK_RAW;
    mask_kind = !has_mask ? M0_ROWPACK_MASK_NONE
              : (row_kind == M0_ROWPACK_PACKED && status == M0_DECODE_OK) ? M0_ROWPACK_MASK_LEGAL : M0_ROWPACK_MASK_LIST;
}

// ---- the position ----
// the eight bytes behind the bitboards as one word (byte 0 = turn), as the kernel's lane 12 stores them
M0_HD uint64_t pos_tail(const Pos& p, int row_kind, int mask_kind) {
    return (uint64_t)p.turn | (uint64_t)(p.cr & 15) << 8 | (uint64_t)(p.ep < 0 ? 255 : p.ep) << 16 | (uint64_t)(p.halfmove & 255) << 24 |
           (uint64_t)(p.fullmove & 255) << 32 | (uint64_t)row_kind << 40 | (uint64_t)mask_kind << 48;
}
// word w of a PACKED row's m0_rowpack_pos (0 .. 11 the men, 12 the tail); p is a decoded position: cr is clean, counters capped
M0_HD uint64_t packed_word(const Pos& p, int mask_kind, int w) {
    if (w == 12) return pos_tail(p, M0_ROWPACK_PACKED, mask_kind);
    return p.bb[w % 6] & p.occ[w < 6 ? m0::WHITE : m0::BLACK];
}
M0_HD uint64_t raw_word(int mask_kind, int w) { return w == 12 ? (uint64_t)M0_ROWPACK_RAW << 40 | (uint64_t)mask_kind << 48 : 0ull; }

// The position of a PACKED row through the decoder's own checks (pos_from_plane_bits: clashes, kings, pawn ranks, cleaned castling,
// the side not to move in check, the move-list bound), so that what reaches the encoder and the move generator is what a decode
// could have produced.  M0_DECODE_OK, or why not (-1: a field out of range).
M0_HD int unpack_pos(const m0_rowpack_pos& q, Pos& p) {
    if (q.turn > 1 || q.castling > 15 || q.halfmove > 99 || q.fullmove > 199 || q.reserved != 0) return -1;
    if (q.ep != 255 && (q.ep >> 3) != (q.turn == m0::WHITE ? 5 : 2)) return -1;
    m0::PlaneBits b;
    for (int k = 0; k < 12; ++k) b.pc[k] = q.men[k];
    b.bad_piece_value = false; b.not_uniform = false;
    b.c7[0] = q.turn ? 1.f : 0.f;
    for (int i = 0; i < 4; ++i) b.c7[1 + i] = (q.castling >> i & 1) ? 1.f : 0.f;
    b.c7[5] = (float)((double)q.halfmove / 99.0);
    b.c7[6] = (float)((double)q.fullmove / 199.0);
    int flags = 0;
    const int st = m0::pos_from_plane_bits(b, p, flags);
    if (st != M0_DECODE_OK) return st;
    p.ep = q.ep == 255 ? (int8_t)-1 : (int8_t)q.ep;
    return M0_DECODE_OK;
}

// ---- 16-byte pieces ----
// which of a pi piece's four floats are entries (bit j = float j): the bit pattern is not zero
M0_HD int pi_piece_bits(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3) {
    return (w0 != 0u ? 1 : 0) | (w1 != 0u ? 2 : 0) | (w2 != 0u ? 4 : 0) | (w3 != 0u ? 8 : 0);
}
// which of a mask piece's sixteen bytes are set (bit j = byte j, little endian words); other: some byte is neither 0 nor 1
M0_HD int mask_piece_bits(const uint32_t w[4], bool& other) {
    int bits = 0;
    for (int j = 0; j < 16; ++j) {
        const uint32_t v = w[j >> 2] >> ((j & 3) * 8) & 255u;
        bits |= (v != 0u ? 1 : 0) << j;
        other = other || v > 1u;
    }
    return bits;
}
// Column order inside a sweep is lane-major: the entries of lane 0's piece, then lane 1's.  With ballot[j] = the lanes whose
// float j is an entry, the place of lane `lane`'s float j among the sweep's entries:
M0_HD int pi_slot(const uint64_t ballot[4], int bits, int lane, int j) {
    const uint64_t below = lane ? ~0ull >> (64 - lane) : 0ull;
    return m0::popc(ballot[0] & below) + m0::popc(ballot[1] & below) + m0::popc(ballot[2] & below) + m0::popc(ballot[3] & below) +
           m0::popc((uint64_t)(bits & ((1 << j) - 1)));
}

// Unpacking walks a row's entries once, in order, sweep by sweep: an entry at column c belongs to sweep c / (64 * per), lane
// c / per % 64, place c % per of that lane's piece (per = 4 floats of pi, 16 bytes of a mask).
M0_HD int entry_sweep(int c, int per) { return c / (LANES * per); }
M0_HD int entry_lane(int c, int per) { return c / per % LANES; }

}  // namespace m0rowpack
