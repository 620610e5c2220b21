// ssl_score_kernel: the SSL losses of stored rows on the device (include/m0_ssl_score.h; the arithmetic is ssl_score_core.h and
// ssl_targets_core.h).  One wave64 per row, ROWS_PER_WG rows per workgroup, lane = tensor square.  A lane reads its square of
// every head channel, of planes 0-12 and, when targets are stored, of their 17 maps: each load of the wave is one 256-byte line.
// The board goes to every lane as four ballots (m0ssl::Board4), so the targets of the planes are made in registers; the 64
// squares are merged by a fixed shuffle tree (lane i takes lane i + 32, then + 16, ... + 1; lane 0 holds the row), and lane 0
// stores the row's 16 columns as four 16-byte stores.  No atomics, no LDS, no workgroup barrier: a row's result is a function of
// that row alone, whatever B, the row's index or the run.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ssl_score_core.h"
#include "ssl_score_kernels.h"

using namespace m0sslscore;

namespace {

constexpr int ROWS_PER_WG = 4;

__global__ __launch_bounds__(ROWS_PER_WG * LANES) void ssl_score_kernel(const float* __restrict__ heads, int tasks, int channels,
                                                                       const float* __restrict__ planes,
                                                                       const float* __restrict__ targets, int B,
                                                                       float* __restrict__ rows) {
    const int lane = threadIdx.x % LANES;
    const int row = blockIdx.x * ROWS_PER_WG + threadIdx.x / LANES;
    if (row >= B) return;                                   // the whole wave: nothing below synchronises across waves
    const float* prow = planes + (size_t)row * M0_PLANES * 64;
    const Logits z = load_logits(tasks, heads + (size_t)row * channels * 64, lane);
    const bool stored = targets != nullptr;

    bool bad;
    const int piece = m0ssl::plane_piece(prow, lane, &bad);
    const float side = prow[12 * 64 + lane], side0 = __shfl(side, 0, LANES);
    const bool unusable = __any(bad || m0ssl::side_bad(side, side0)) != 0;
    const bool poisoned = __any(!(poison_of(z) == 0.f)) != 0;

    Targets own = {};
    if (!unusable) {                                        // (uniform)
        m0ssl::Board4 board;
#pragma unroll
        for (int j = 0; j < 4; ++j) board.w[j] = __ballot(((piece + 1) >> j) & 1);
        own = targets_of(m0ssl::square_targets(board, lane, side0 == 1.f));
    }
    Targets t = own;
    bool differ = false;
    if (stored) {
        t = stored_targets(targets + (size_t)row * m0ssl::TARGET_CH * 64, lane);
        differ = __any(classes_differ(tasks, t, own)) != 0;
    }

    Cell cell;
    if (stored || !unusable) cell = score_square(tasks, z, t);
#pragma unroll
    for (int off = LANES / 2; off > 0; off >>= 1) {
        Cell o;
#pragma unroll
        for (int i = 0; i < 5; ++i) o.loss[i] = __shfl_down(cell.loss[i], off, LANES);
#pragma unroll
        for (int i = 0; i < COUNTS; ++i) o.n[i] = __shfl_down(cell.n[i], off, LANES);
        if (lane < off) cell.merge(o);
    }

    if (lane == 0) {
        float out[M0_SSL_SCORE_COLS];
        finish(cell, unusable, poisoned, stored, differ, out);
        float4* dst = reinterpret_cast<float4*>(rows + (size_t)row * M0_SSL_SCORE_COLS);
#pragma unroll
        for (int q = 0; q < 4; ++q) dst[q] = make_float4(out[4 * q], out[4 * q + 1], out[4 * q + 2], out[4 * q + 3]);
    }
}

}  // namespace

hipError_t launch_ssl_score(const float* heads, int tasks, const float* planes, const float* targets, int B, float* rows,
                            hipStream_t stream) {
    const int grid = (B + ROWS_PER_WG - 1) / ROWS_PER_WG;
    ssl_score_kernel<<<grid, ROWS_PER_WG * LANES, 0, stream>>>(heads, tasks, channels(tasks), planes, targets, B, rows);
    return hipGetLastError();
}
