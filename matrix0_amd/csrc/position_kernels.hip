// Position-wise kernels outside the search, one wave per position:
//   encode_positions_kernel  encoding.py on device (planes, NHWC input, legal moves, policy indices, mask): parity tests and
//                            boundary helpers; shares the move generator and the encoder with select_kernel.
//   ssl_targets_kernel       self-supervised training targets of recorded positions (ssl_targets_core.h).
//   ssl_targets_planes_kernel  the same targets of stored planes, without a Pos.
//   decode_planes_kernel     the way back: stored planes (and legal mask) -> position, checked (planes_decode.h).
#include <hip/hip_runtime.h>
#include "tree.h"
#include "movegen_wave.h"
#include "planes_decode.h"
#include "ssl_targets_core.h"

using namespace m0;

// ---- position-wise encoding.py on device: one wave per position ----
__global__ __launch_bounds__(64) void encode_positions_kernel(const Pos* pos, int n, float* planes, _Float16* nhwc,
                                                              uint8_t* mask, int32_t* nlegal, uint16_t* moves, int32_t* idxs) {
    __shared__ Move smoves[M0_MAX_MOVES];
    __shared__ Move spseudo[M0_MAX_MOVES];
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= n) return;
    const Pos p = pos[i];
    if (planes) {
        float c7[7];
        plane_consts(p, c7);
        const int s = (7 - (lane >> 3)) * 8 + (lane & 7);
        const int pl = piece_plane(p, s);
        float* o = planes + (size_t)i * M0_PLANES * 64;
        for (int k = 0; k < 12; ++k) o[k * 64 + lane] = pl == k ? 1.f : 0.f;
        for (int k = 0; k < 7; ++k) o[(12 + k) * 64 + lane] = c7[k];
    }
    if (nhwc) encode_nhwc(p, nhwc_row(nhwc, i), lane);
    const int k = gen_legal_wave(p, smoves, spseudo, lane);   // the search's generator (same list as gen_legal)
    __syncthreads();
    if (mask) for (int j = lane; j < M0_POLICY_SIZE; j += 64) mask[(size_t)i * M0_POLICY_SIZE + j] = 0;
    __syncthreads();
    for (int j = lane; j < M0_MAX_MOVES; j += 64) {
        int idx = -1;
        Move m = 0;
        if (j < k) { m = smoves[j]; idx = move_to_index(p, m); if (mask && idx >= 0) mask[(size_t)i * M0_POLICY_SIZE + idx] = 1; }
        if (moves) moves[(size_t)i * M0_MAX_MOVES + j] = m;
        if (idxs) idxs[(size_t)i * M0_MAX_MOVES + j] = idx;
    }
    if (lane == 0 && nlegal) nlegal[i] = k;
}

hipError_t launch_encode_positions(const Pos* pos_dev, int n, float* planes, _Float16* nhwc, uint8_t* mask,
                                   int32_t* nlegal, uint16_t* moves, int32_t* idxs, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(encode_positions_kernel, dim3(n), dim3(64), 0, st, pos_dev, n, planes, nhwc, mask, nlegal, moves, idxs);
    return hipGetLastError();
}

// ---- SSL training targets (azchess/ssl_algorithms.py:51-143, 256-557), one wave per position, lane = tensor square; the
// per-square arithmetic is ssl_targets_core.h.  out f32 [n][17][64]: piece one-hot (13), threat, pin, fork, control.
__global__ __launch_bounds__(64) void ssl_targets_kernel(const Pos* pos, int n, float* out) {
    __shared__ int8_t pc[64];          // plane index 0..11 (white P..K, black P..K) or -1, by tensor square
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= n) return;
    const Pos p = pos[i];
    pc[lane] = (int8_t)piece_plane(p, (7 - (lane >> 3)) * 8 + (lane & 7));
    __syncthreads();
    const m0ssl::SquareTargets t = m0ssl::square_targets([&](int sq) -> int { return pc[sq]; }, lane, p.turn == WHITE);
    m0ssl::store_square(t, out + (size_t)i * m0ssl::TARGET_CH * 64, lane);
}

hipError_t launch_ssl_targets(const Pos* pos_dev, int n, float* out_dev, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(ssl_targets_kernel, dim3(n), dim3(64), 0, st, pos_dev, n, out_dev);
    return hipGetLastError();
}

// ---- the same maps from stored planes, one wave per row: the lanes read their square of planes 0-12, four ballots make the
// board (m0ssl::Board4), and an unusable row (ssl_targets_core.h) gets status 1 and no targets.  No shared memory.
__global__ __launch_bounds__(64) void ssl_targets_planes_kernel(const float* planes, int n, float* out, int32_t* status) {
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= n) return;
    const float* row = planes + (size_t)i * M0_PLANES * 64;
    bool bad;
    const int piece = m0ssl::plane_piece(row, lane, &bad);
    const float side = row[12 * 64 + lane], side0 = __shfl(side, 0);
    const bool unusable = __any(bad || m0ssl::side_bad(side, side0)) != 0;
    if (lane == 0) status[i] = unusable ? 1 : 0;
    if (unusable) return;
    m0ssl::Board4 board;
    for (int j = 0; j < 4; ++j) board.w[j] = __ballot(((piece + 1) >> j) & 1);
    m0ssl::store_square(m0ssl::square_targets(board, lane, side0 == 1.f), out + (size_t)i * m0ssl::TARGET_CH * 64, lane);
}

hipError_t launch_ssl_targets_planes(const float* planes_dev, int n, float* out_dev, int32_t* status_dev, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(ssl_targets_planes_kernel, dim3(n), dim3(64), 0, st, planes_dev, n, out_dev, status_dev);
    return hipGetLastError();
}

// ---- stored planes -> position (planes_decode.h), one wave per row, lane = tensor square.  A ballot per piece plane is that
// plane's bitboard in tensor order (rank 8 first); a byte swap turns it into Pos order (a1 = bit 0).  The seven constant planes
// must be uniform over the lanes: one ballot each.  The decoded position's legal moves come from the search's generator
// (the two LDS lists of encode_positions_kernel); with a mask they must set exactly its bits.  Nothing is shared between
// waves, no atomics.  Every read stays inside the row: planes and mask are indexed by lane / a strided loop only, except
// ep_from_mask and the legal moves' indices, both bounded to [0, M0_POLICY_SIZE) before use.
__global__ __launch_bounds__(64) void decode_planes_kernel(const float* planes, const uint8_t* mask, int n, Pos* pos,
                                                           int32_t* status, int32_t* flags, int32_t* nlegal) {
    __shared__ Move smoves[M0_MAX_MOVES];
    __shared__ Move spseudo[M0_MAX_MOVES];
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= n) return;
    const float* row = planes + (size_t)i * M0_PLANES * 64;
    const uint8_t* mrow = mask ? mask + (size_t)i * M0_POLICY_SIZE : nullptr;
    PlaneBits b;
    bool bad = false;
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        const uint32_t u = f32_bits(row[k * 64 + lane]);
        b.pc[k] = __builtin_bswap64(__ballot(u == 0x3f800000u));
        bad = bad || (u != 0u && u != 0x3f800000u);
    }
    b.bad_piece_value = __any(bad);
    b.not_uniform = false;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        const float v = row[(12 + k) * 64 + lane];
        b.c7[k] = __shfl(v, 0);
        b.not_uniform = b.not_uniform || __ballot(f32_bits(v) != f32_bits(b.c7[k])) != 0ull;
    }
    Pos p;
    int fl = mrow ? 0 : M0_DECODE_NO_MASK;
    int st = pos_from_plane_bits(b, p, fl);                            // uniform: every lane holds the same planes
    int k = 0;
    if (st == M0_DECODE_OK) {                                          // (uniform branch: the generator synchronises)
        if (mrow) {
            const int ep = ep_from_mask(p, mrow);
            if (ep >= 0) { p.ep = (int8_t)ep; fl |= M0_DECODE_EP_FROM_MASK; }
        }
        k = gen_legal_wave(p, smoves, spseudo, lane);
        if (mrow) {
            // the legal moves' indices are distinct: equal masks = every one of them set and as many bytes set as moves
            int set = 0;
            for (int j = lane; j < M0_POLICY_SIZE; j += 64) set += mrow[j] ? 1 : 0;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) set += __shfl_xor(set, off);
            bool miss = false;
            for (int j = lane; j < k; j += 64) {
                const int idx = move_to_index(p, smoves[j]);
                miss = miss || idx < 0 || idx >= M0_POLICY_SIZE || !mrow[idx];
            }
            if (__any(miss) || set != k) st = M0_DECODE_MASK_MISMATCH;
        }
    } else {
        for (int t = 0; t < 6; ++t) p.bb[t] = 0;
        p.occ[0] = p.occ[1] = 0;
        p.turn = 0; p.cr = 0; p.ep = 0; p.pad = 0; p.halfmove = 0; p.fullmove = 0;
    }
    if (lane == 0) { pos[i] = p; status[i] = st; flags[i] = fl; nlegal[i] = k; }
}

hipError_t launch_decode_planes(const float* planes_dev, const uint8_t* mask_dev, int n, Pos* pos_dev, int32_t* status_dev,
                                int32_t* flags_dev, int32_t* nlegal_dev, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(decode_planes_kernel, dim3(n), dim3(64), 0, st, planes_dev, mask_dev, n, pos_dev, status_dev, flags_dev, nlegal_dev);
    return hipGetLastError();
}
