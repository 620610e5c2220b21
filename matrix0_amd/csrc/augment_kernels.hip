// augment_rows_kernel: the trainer's flip and rotate augmentations of stored rows on the device (include/m0_augment.h; the maps
// are augment_core.h).  A pure permutation of a row's own cells: a gather on the read side, contiguous 16-byte stores on the write
// side.  A workgroup of 256 threads first writes, for both transforming kinds, the source column of each of the 4672 output columns
// into LDS (m0aug::source_column, 2 x 4672 u16), then walks rows blockIdx.x, + gridDim.x, ...: for a row of kind k, thread t takes
// the 16-byte output pieces t, t + 256, ... of
//   pi     1168 pieces of 4 floats: one 8-byte LDS read gives the 4 source columns, 4 dword loads, one float4 store
//   mask    292 pieces of 16 bytes: 16 byte loads, one uint4 store (4672 = 73 * 64 is 16 * 292, no multiple of 256: the last
//           sweep of either loop is partial)
//   planes P * 16 pieces: 4 neighbouring files of one rank are read from 4 neighbouring files (the map of the squares is an XOR with
//           7 or 63), so one float4 load at the mirrored piece, its components reversed
// and a row of kind M0_AUG_NONE is copied piece by piece.  A row is read once from HBM (its 28 KB stay in the caches between the
// gathers of neighbouring pieces) and written once.  No atomics, no state across rows: an output row is a function of its input
// row and its kind, whatever B, the row's index or the grid.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "augment_core.h"
#include "augment_kernels.h"

using namespace m0aug;

namespace {

constexpr int THREADS = 256;
constexpr int MAX_GRID = 2048;                       // 256 CUs x 8 workgroups; the rows beyond are walked by stride
constexpr int PI_PIECES = COLS / 4;                  // 1168
constexpr int MASK_PIECES = COLS / 16;               // 292
static_assert(COLS % 16 == 0, "rows are whole 16-byte pieces");

__global__ __launch_bounds__(THREADS) void augment_rows_kernel(const float* __restrict__ s, const float* __restrict__ pi,
                                                               const uint8_t* __restrict__ mask, const uint8_t* __restrict__ kinds,
                                                               int uniform_kind, int B, int P, float* __restrict__ s_out,
                                                               float* __restrict__ pi_out, uint8_t* __restrict__ mask_out) {
    __shared__ __attribute__((aligned(16))) uint16_t from[2][COLS];      // [kind - 1][output column] -> source column
    for (int col = threadIdx.x; col < COLS; col += THREADS) {
        from[0][col] = (uint16_t)source_column(M0_AUG_HFLIP, col);
        from[1][col] = (uint16_t)source_column(M0_AUG_ROT180, col);
    }
    __syncthreads();

    const int plane_pieces = P * (SQUARES / 4);
    for (int row = blockIdx.x; row < B; row += gridDim.x) {
        int kind = kinds ? (int)kinds[row] : uniform_kind;           // uniform over the workgroup
        if (!valid_kind(kind)) kind = M0_AUG_NONE;
        const float* srow = s + (size_t)row * P * SQUARES;
        const float* prow = pi + (size_t)row * COLS;
        float4* sdst = reinterpret_cast<float4*>(s_out + (size_t)row * P * SQUARES);
        float4* pdst = reinterpret_cast<float4*>(pi_out + (size_t)row * COLS);
        const uint8_t* mrow = mask ? mask + (size_t)row * COLS : nullptr;
        uint4* mdst = mask ? reinterpret_cast<uint4*>(mask_out + (size_t)row * COLS) : nullptr;

        if (kind == M0_AUG_NONE) {
            for (int j = threadIdx.x; j < plane_pieces; j += THREADS) sdst[j] = reinterpret_cast<const float4*>(srow)[j];
            for (int j = threadIdx.x; j < PI_PIECES; j += THREADS) pdst[j] = reinterpret_cast<const float4*>(prow)[j];
            if (mrow)
                for (int j = threadIdx.x; j < MASK_PIECES; j += THREADS) mdst[j] = reinterpret_cast<const uint4*>(mrow)[j];
            continue;
        }

        // planes: piece j holds squares 4j .. 4j + 3 of plane j / 16; their sources are the squares 4 (j ^ x) + 3 .. 4 (j ^ x),
        // x = 1 (the other half of the rank) or 15 (the rotated half-rank of the same plane)
        const int piece_xor = map_square(kind, 0) >> 2;
        for (int j = threadIdx.x; j < plane_pieces; j += THREADS) {
            const float4 v = reinterpret_cast<const float4*>(srow)[j ^ piece_xor];
            sdst[j] = make_float4(v.w, v.z, v.y, v.x);
        }
        const uint16_t* tab = from[kind - 1];
        for (int j = threadIdx.x; j < PI_PIECES; j += THREADS) {
            const ushort4 c = reinterpret_cast<const ushort4*>(tab)[j];
            pdst[j] = make_float4(prow[c.x], prow[c.y], prow[c.z], prow[c.w]);
        }
        if (mrow) {
            for (int j = threadIdx.x; j < MASK_PIECES; j += THREADS) {
                const uint4 lo = reinterpret_cast<const uint4*>(tab)[2 * j], hi = reinterpret_cast<const uint4*>(tab)[2 * j + 1];
                const uint32_t c[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};        // two source columns in each
                uint32_t w[4];
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    w[k] = (uint32_t)mrow[c[2 * k] & 0xffffu] | (uint32_t)mrow[c[2 * k] >> 16] << 8 |
                           (uint32_t)mrow[c[2 * k + 1] & 0xffffu] << 16 | (uint32_t)mrow[c[2 * k + 1] >> 16] << 24;
                mdst[j] = make_uint4(w[0], w[1], w[2], w[3]);
            }
        }
    }
}

}  // namespace

hipError_t launch_augment_rows(const float* s, const float* pi, const uint8_t* mask, const uint8_t* kinds, int uniform_kind, int B, int P,
                               float* s_out, float* pi_out, uint8_t* mask_out, hipStream_t stream) {
    if (!s || !pi || !s_out || !pi_out || B <= 0 || P <= 0) return hipErrorInvalidValue;
    if ((mask != nullptr) != (mask_out != nullptr)) return hipErrorInvalidValue;
    if (s == s_out || pi == pi_out || (mask && mask == mask_out)) return hipErrorInvalidValue;
    if (!kinds && !valid_kind(uniform_kind)) return hipErrorInvalidValue;
    const int grid = B < MAX_GRID ? B : MAX_GRID;
    augment_rows_kernel<<<grid, THREADS, 0, stream>>>(s, pi, mask, kinds, uniform_kind, B, P, s_out, pi_out, mask_out);
    return hipGetLastError();
}
