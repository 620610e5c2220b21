// Per-row rules of a training batch read from resident packed rows (include/m0_batch.h), host and device: batch_kernels.hip runs
// them one wave per output row, batch_host.h runs them on the CPU with plain loops (m0_rowstore_batch_host and the host store).
// An output row is the packed row expanded (rowpack_core.h) and then transformed by the trainer's augmentation (augment_core.h),
// written in one go: where each entry lands and what each plane cell shows is decided here, once.
//
//   planes  output cell t of plane k shows the source cell map_square(kind, t); for a PACKED row that is the encoder's arithmetic
//           (plane_consts, piece_plane of chess_core.h) on the chess square of that cell.
//   pi      out[col] = in[source_column(kind, col)].  The maps are involutions, so an entry at column c lands at
//           dest_column(kind, c) = source_column(kind, c): a scatter of the entries over zeros, no gather over 4672 columns.
//   masks   as pi: LIST entries and the indices of the legal moves go through dest_column.
//   RAW     rows are moved from the segment's dense arrays by the read-side rule, as augment_rows_kernel moves them.
//   ssl     (include/m0_batch_ssl.h, when asked for) the target maps of the OUTPUT planes, f32 [17][64]: cell t of every map is
//           m0ssl::square_targets at tensor square t of the board whose square t holds the piece output cell t shows, with the
//           side to move the output planes show.  Nothing is computed for the stored row and moved afterwards: the reference's
//           pawn attacks point one way in tensor space, so the maps of rotated planes are not the rotated maps.
//             PACKED  the piece on cell t is piece_plane at cell_square(kind, t), the value the planes are written from, and the
//                     side to move is the position's; the row is a position, so its status is 0.
//             RAW     the piece on cell t is m0ssl::plane_piece of the stored planes at map_square(kind, t) (raw_cell), and
//                     plane 12 there is held against plane 12 of output cell 0.  One bad cell makes the row unusable
//                     (ssl_targets_core.h): status 1 and all 17 maps zero (zero_cell).  Otherwise status 0.
#pragma once
#include <stdint.h>
#include "../../include/m0_engine.h"
#include "augment_core.h"
#include "rowpack_core.h"
#include "ssl_targets_core.h"

namespace m0batch {

using m0::Pos;
using m0rowpack::COLS;
using m0rowpack::PLANE_FLOATS;

// One segment's arrays, all in host memory or all in device memory: the arrays of m0_rowpack_arrays behind check_arrays, with the
// engine's positions (the filler for RAW rows) and the RAW rows' slots that the check produced, and the two kinds of a row as
// one byte.  A device segment begins with its own SegView, so a row reference needs no table of segments.
struct SegView {
    int64_t n;
    const Pos* pos;                 // [n]
    const uint8_t* meta;            // [n] row_kind | mask_kind << 1
    const float* z;                 // [n]
    const int64_t* pi_off;          // [n + 1]
    const uint16_t* pi_idx;
    const float* pi_val;
    const int64_t* mask_off;        // [n + 1]
    const uint16_t* mask_idx;
    const int32_t* raw_slot;        // [n], -1 for PACKED rows
    const float* raw_planes;        // [raw][19 * 64]
    const float* raw_pi;            // [raw][4672]
    const uint8_t* raw_mask;        // [raw][4672], null without masks
};

// Output row b of a batch: row `row` of segment `seg` under augmentation `kind`
struct RowRef {
    const SegView* seg;
    int32_t row;
    int32_t kind;
};
static_assert(sizeof(RowRef) == 16, "a row reference is one 16-byte piece of the per-batch descriptor");

M0_HD uint8_t make_meta(int row_kind, int mask_kind) { return (uint8_t)(row_kind | mask_kind << 1); }
M0_HD bool meta_raw(uint8_t meta) { return (meta & 1) == M0_ROWPACK_RAW; }
M0_HD int meta_mask_kind(uint8_t meta) { return meta >> 1; }

// where the entry of source column `col` (pi or mask) lands in a row of this kind
M0_HD int dest_column(int kind, int col) { return m0aug::source_column(kind, col); }
// the chess square (a1 = 0) that output plane cell t (row-major, row 0 = rank 8) of a row of this kind shows
M0_HD int cell_square(int kind, int t) {
    const int u = m0aug::map_square(kind, t);
    return (7 - (u >> 3)) * 8 + (u & 7);
}
// plane k of a cell whose square holds piece plane pl (-1: empty), with the position's seven constants
M0_HD float plane_cell(int pl, const float* c7, int k) {
    float v = pl == k ? 1.f : 0.f;
    for (int i = 0; i < 7; ++i) v = k == 12 + i ? c7[i] : v;
    return v;
}

// ---- the SSL target maps of an output row
constexpr int SSL_FLOATS = m0ssl::TARGET_CH * 64;
static_assert(m0ssl::TARGET_CH == M0_BATCH_SSL_CH, "a row of maps is the row of ssl_targets_core.h");

// RAW row: the piece that output cell t of a row of this kind shows, from the stored planes f32 [19][64]; *bad when the cell makes
// the row unusable (a piece-plane value that is neither 0 nor 1, two pieces, or a plane 12 that is not output cell 0's 0 or 1)
M0_HD int raw_cell(const float* stored, int kind, int t, bool* bad) {
    const int u = m0aug::map_square(kind, t);
    bool off;
    const int piece = m0ssl::plane_piece(stored, u, &off);
    *bad = off || m0ssl::side_bad(stored[12 * 64 + u], stored[12 * 64 + m0aug::map_square(kind, 0)]);
    return piece;
}
// RAW row: whether the output planes show white to move
M0_HD bool raw_white(const float* stored, int kind) { return stored[12 * 64 + m0aug::map_square(kind, 0)] == 1.f; }
// cell t of the 17 maps of a usable row from the board of its output cells, and of an unusable row
template <class Board>
M0_HD void target_cell(const Board& board, int t, bool stm_white, float* maps) {
    m0ssl::store_square(m0ssl::square_targets(board, t, stm_white), maps, t);
}
M0_HD void zero_cell(float* maps, int t) {
    for (int k = 0; k < m0ssl::TARGET_CH; ++k) maps[k * 64 + t] = 0.f;
}

}  // namespace m0batch
