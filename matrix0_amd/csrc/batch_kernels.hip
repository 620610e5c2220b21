// batch_rows_kernel: a training batch from resident packed rows in one launch (include/m0_batch.h; the per-row rules are
// batch_core.h).  Output row b is row `row` of segment `seg` expanded as rowpack_unpack_kernel behind encode_positions_kernel
// expands it and transformed as augment_rows_kernel transforms it, but written once: the transform is applied where an entry
// lands, not to a dense row.
//
// One wave64 per output row, one row per workgroup (gen_legal_wave synchronises the workgroup, and rows of different kinds take
// different paths).  For a PACKED row:
//   planes  lane t holds the piece plane of output cell t (piece_plane at cell_square(kind, t)); the lane that owns 16-byte piece
//           j = plane j / 16, cells 4 (j % 16) .. + 3 fetches those four lanes' values once and stores 19 planes as 304 pieces.
//   pi      built in LDS (4672 words): zeroed with 16-byte writes, the row's entries scattered to dest_column(kind, column),
//           then streamed out as 1168 pieces.
//   mask    built in LDS (4672 bytes) in the same way from the LIST entries, or from the legal moves of the position
//           (gen_legal_wave, move_to_index); streamed out as 292 pieces.
// A RAW row is gathered from the segment's dense arrays by the read-side rule (source_column, map_square), a piece per lane.
// Every byte of planes, pi and mask is written exactly once, with 16-byte stores; z is the one dword a row has.  No atomics,
// nothing shared between waves: a row's bytes depend on (seg, row, kind) alone.  LDS: 18 688 + 4 672 + 2 x 512 bytes a workgroup,
// six workgroups on a CU's 160 KB.
//
// SSL = true (include/m0_batch_ssl.h) is the same body with two more outputs, the target maps of the row's output planes and
// their status (the rule: batch_core.h); SSL = false compiles to the kernel without them.  Lane t owns output cell t:
//   PACKED  four ballots of the piece plane the lane already holds make the board (m0ssl::Board4); the side to move is the
//           position's.  No LDS, no global read.
//   RAW     the lane reads its cell of planes 0-12 of the stored row by the read-side rule (raw_cell); one __any decides for the
//           wave whether the row is usable.  An unusable row gets zeros.
// A wave stores each of the 17 maps as one whole 256-byte row (lane t the dword of cell t), so every byte of ssl[b] is written
// exactly once; ssl_status[b] is one dword from lane 0.  No LDS is added.
//
// Bounds: the host has checked b < B, row < seg->n and kind <= 2.  check_arrays has run over every segment: an entry's column is
// below 4672, dest_column maps [0, 4672) onto itself, so a scatter stays inside the workgroup's own LDS arrays; a row reads
// [off[row], off[row + 1]) of its segment's entries only; raw_slot of a RAW row is below the segment's RAW rows.  A move index is
// bounded before it is used.  Global stores go to pieces below PLANE_PIECES, PI_PIECES and MASK_PIECES of row b.  The maps go to
// ssl + b * 17 * 64 + k * 64 + lane with k < 17 and lane < 64; raw_cell reads planes 0-12 of the RAW row's own slot at squares
// below 64 (map_square maps [0, 64) onto itself).
#include <hip/hip_runtime.h>
#include "batch_core.h"
#include "batch_kernels.h"
#include "movegen_wave.h"

using namespace m0batch;
using m0rowpack::LANES;
using m0rowpack::MASK_PIECES;
using m0rowpack::PI_PIECES;
using m0rowpack::PLANE_PIECES;

namespace {

template <bool SSL>
__global__ __launch_bounds__(LANES) void batch_rows_kernel(const RowRef* __restrict__ refs, int B, float* __restrict__ planes,
                                                          float* __restrict__ pi, float* __restrict__ z, uint8_t* __restrict__ mask,
                                                          float* __restrict__ ssl, int32_t* __restrict__ ssl_status) {
    __shared__ __attribute__((aligned(16))) uint32_t spi[COLS];
    __shared__ __attribute__((aligned(16))) uint8_t smask[COLS];
    __shared__ Move smoves[M0_MAX_MOVES];
    __shared__ Move spseudo[M0_MAX_MOVES];
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= B) return;
    const RowRef ref = refs[b];
    const SegView& g = *ref.seg;
    const int row = ref.row, kind = ref.kind;
    uint4* sdst = reinterpret_cast<uint4*>(planes + (size_t)b * PLANE_FLOATS);
    uint4* pdst = reinterpret_cast<uint4*>(pi + (size_t)b * COLS);
    uint4* mdst = mask ? reinterpret_cast<uint4*>(mask + (size_t)b * COLS) : nullptr;
    if (lane == 0) z[b] = g.z[row];
    const uint8_t meta = g.meta[row];

    if (meta_raw(meta)) {                                                 // uniform: one row per workgroup
        const size_t slot = (size_t)g.raw_slot[row];
        const uint32_t* rs = reinterpret_cast<const uint32_t*>(g.raw_planes + slot * PLANE_FLOATS);
        const uint32_t* rp = reinterpret_cast<const uint32_t*>(g.raw_pi + slot * COLS);
        if constexpr (SSL) {
            const float* stored = g.raw_planes + slot * PLANE_FLOATS;
            float* maps = ssl + (size_t)b * SSL_FLOATS;
            bool bad;
            const int piece = raw_cell(stored, kind, lane, &bad);
            const bool unusable = __any(bad) != 0;                        // once per wave
            if (lane == 0) ssl_status[b] = unusable ? 1 : 0;
            if (unusable) {
                zero_cell(maps, lane);
            } else {
                m0ssl::Board4 board;
                for (int j = 0; j < 4; ++j) board.w[j] = __ballot(((piece + 1) >> j) & 1);
                target_cell(board, lane, raw_white(stored, kind), maps);
            }
        }
        for (int j = lane; j < PLANE_PIECES; j += LANES) {
            const uint32_t* src = rs + (j >> 4) * 64;
            const int t = (j & 15) * 4;
            sdst[j] = make_uint4(src[m0aug::map_square(kind, t)], src[m0aug::map_square(kind, t + 1)], src[m0aug::map_square(kind, t + 2)],
                                 src[m0aug::map_square(kind, t + 3)]);
        }
        for (int j = lane; j < PI_PIECES; j += LANES)
            pdst[j] = make_uint4(rp[m0aug::source_column(kind, 4 * j)], rp[m0aug::source_column(kind, 4 * j + 1)],
                                 rp[m0aug::source_column(kind, 4 * j + 2)], rp[m0aug::source_column(kind, 4 * j + 3)]);
        if (mask) {
            const uint8_t* rm = g.raw_mask + slot * COLS;
            for (int j = lane; j < MASK_PIECES; j += LANES) {
                uint32_t w[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int c = 16 * j + 4 * k;
                    w[k] = (uint32_t)rm[m0aug::source_column(kind, c)] | (uint32_t)rm[m0aug::source_column(kind, c + 1)] << 8 |
                           (uint32_t)rm[m0aug::source_column(kind, c + 2)] << 16 | (uint32_t)rm[m0aug::source_column(kind, c + 3)] << 24;
                }
                mdst[j] = make_uint4(w[0], w[1], w[2], w[3]);
            }
        }
        return;
    }

    const Pos p = g.pos[row];
    // ---- planes: registers only ----
    {
        float c7[7];
        plane_consts(p, c7);
        const int pl = piece_plane(p, cell_square(kind, lane));
        if constexpr (SSL) {
            m0ssl::Board4 board;
            for (int j = 0; j < 4; ++j) board.w[j] = __ballot(((pl + 1) >> j) & 1);
            target_cell(board, lane, p.turn == WHITE, ssl + (size_t)b * SSL_FLOATS);
            if (lane == 0) ssl_status[b] = 0;
        }
        int pl4[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) pl4[i] = __shfl(pl, (lane & 15) * 4 + i);
        for (int j = lane; j < PLANE_PIECES; j += LANES) {
            const int k = j >> 4;
            sdst[j] = make_uint4(__float_as_uint(plane_cell(pl4[0], c7, k)), __float_as_uint(plane_cell(pl4[1], c7, k)),
                                 __float_as_uint(plane_cell(pl4[2], c7, k)), __float_as_uint(plane_cell(pl4[3], c7, k)));
        }
    }
    // ---- pi and the mask: zeros, then the entries where they land, then out ----
    const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
    for (int j = lane; j < PI_PIECES; j += LANES) reinterpret_cast<uint4*>(spi)[j] = zero;
    if (mask)
        for (int j = lane; j < MASK_PIECES; j += LANES) reinterpret_cast<uint4*>(smask)[j] = zero;
    __syncthreads();
    for (int64_t e = g.pi_off[row] + lane, end = g.pi_off[row + 1]; e < end; e += LANES)
        spi[dest_column(kind, g.pi_idx[e])] = __float_as_uint(g.pi_val[e]);
    if (mask) {
        if (meta_mask_kind(meta) == M0_ROWPACK_MASK_LIST) {
            for (int64_t e = g.mask_off[row] + lane, end = g.mask_off[row + 1]; e < end; e += LANES)
                smask[dest_column(kind, g.mask_idx[e])] = 1;
        } else {
            const int k = gen_legal_wave(p, smoves, spseudo, lane);       // synchronises before it returns
            for (int j = lane; j < k; j += LANES) {
                const int idx = move_to_index(p, smoves[j]);
                if (idx >= 0 && idx < COLS) smask[dest_column(kind, idx)] = 1;
            }
        }
    }
    __syncthreads();
    for (int j = lane; j < PI_PIECES; j += LANES) pdst[j] = reinterpret_cast<const uint4*>(spi)[j];
    if (mask)
        for (int j = lane; j < MASK_PIECES; j += LANES) mdst[j] = reinterpret_cast<const uint4*>(smask)[j];
}

}  // namespace

hipError_t launch_batch_rows(const RowRef* refs, int B, float* planes, float* pi, float* z, uint8_t* mask, hipStream_t st) {
    if (!refs || !planes || !pi || !z || B <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(batch_rows_kernel<false>, dim3(B), dim3(LANES), 0, st, refs, B, planes, pi, z, mask, nullptr, nullptr);
    return hipGetLastError();
}

hipError_t launch_batch_rows_ssl(const RowRef* refs, int B, float* planes, float* pi, float* z, uint8_t* mask, float* ssl,
                                 int32_t* ssl_status, hipStream_t st) {
    if (!refs || !planes || !pi || !z || !ssl || !ssl_status || B <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(batch_rows_kernel<true>, dim3(B), dim3(LANES), 0, st, refs, B, planes, pi, z, mask, ssl, ssl_status);
    return hipGetLastError();
}
