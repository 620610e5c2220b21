// Packed training rows on the device (include/m0_rowpack.h, rowpack_core.h): one wave64 per row, four rows per workgroup, a lane
// per 16-byte piece (piece k * 64 + lane in sweep k, the access pattern of score_rows_kernel).  No LDS, no barrier, no atomics and
// nothing shared between waves: what a row writes depends on that row alone.
//
//   rowpack_count_kernel   behind decode_planes_kernel: the row's kinds, its m0_rowpack_pos (lanes 0 .. 12 store a word each)
//                          and how many pi and LIST-mask entries it will store.
//   rowpack_fill_kernel    the entries, compacted in column order: a ballot per float of the piece, popcounts below the lane
//                          (pi); a lane prefix of the pieces' popcounts (masks).  RAW rows copy themselves into the raw arrays.
//   rowpack_unpack_kernel  behind encode_positions_kernel: a row's entries are walked once, 64 at a time in registers; the
//                          lane that owns an entry's piece takes it from a readlane, and every piece leaves as one 16-byte
//                          store, zeros included.
//
// Bounds: every dense access is piece < PIECES of the row's own arrays; a fill writes [off[row], off[row + 1]) only, which the
// count pass sized on the same bytes; an unpack reads [off[row], off[row + 1]) only, and an entry's column decides a LANE and a
// place in that lane's registers, never an address.
#include <hip/hip_runtime.h>
#include "rowpack_core.h"
#include "rowpack_kernels.h"

using namespace m0rowpack;
using m0::Pos;

namespace {

constexpr int ROWS_PER_BLOCK = 4;

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
// exclusive prefix over the lanes; total = the wave's sum
__device__ __forceinline__ int wave_prefix(int v, int lane, int& total) {
    int inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(inc, off);
        if (lane >= off) inc += t;
    }
    total = __shfl(inc, 63);
    return inc - v;
}
__device__ __forceinline__ uint4 load_piece(const void* row, int piece, int pieces) {
    return piece < pieces ? ((const uint4*)row)[piece] : make_uint4(0u, 0u, 0u, 0u);
}
__device__ __forceinline__ void copy_pieces(void* dst, const void* src, int pieces, int lane) {
    for (int p = lane; p < pieces; p += LANES) ((uint4*)dst)[p] = ((const uint4*)src)[p];
}
__device__ __forceinline__ int lane_value(int v, int j) { return __builtin_amdgcn_readlane(v, __builtin_amdgcn_readfirstlane(j)); }

__global__ __launch_bounds__(64 * ROWS_PER_BLOCK) void rowpack_count_kernel(const float* pi, const uint8_t* mask, const Pos* pos,
                                                                           const int32_t* status, int n, m0_rowpack_pos* out_pos,
                                                                           int32_t* counts) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (row >= n) return;
    bool other = false;
    int mcount = 0, pcount = 0;
    if (mask) {
        const uint8_t* mrow = mask + (size_t)row * COLS;
        for (int k = 0; k < MASK_SWEEPS; ++k) {
            const uint4 v = load_piece(mrow, k * LANES + lane, MASK_PIECES);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
            mcount += __popc(mask_piece_bits(w, other));
        }
        other = __any(other) != 0;
    }
    int rk, mk;
    row_kinds(status[row], mask != nullptr, !other, rk, mk);
    if (rk == M0_ROWPACK_PACKED && pi) {
        const float* prow = pi + (size_t)row * COLS;
        for (int k = 0; k < PI_SWEEPS; ++k) {
            const uint4 v = load_piece(prow, k * LANES + lane, PI_PIECES);
            pcount += __popc(pi_piece_bits(v.x, v.y, v.z, v.w));
        }
    }
    pcount = wave_sum(pcount);
    mcount = wave_sum(mcount);
    if (lane < 13)                                             // (the position stays in global memory: a lane reads two words of it)
        ((uint64_t*)(out_pos + row))[lane] = rk == M0_ROWPACK_PACKED ? packed_word(pos[row], mk, lane) : raw_word(mk, lane);
    if (lane == 0) {
        counts[2 * (size_t)row] = pcount;                                                  // 0 for a RAW row: not swept
        counts[2 * (size_t)row + 1] = rk == M0_ROWPACK_PACKED && mk == M0_ROWPACK_MASK_LIST ? mcount : 0;
    }
}

__global__ __launch_bounds__(64 * ROWS_PER_BLOCK) void rowpack_fill_kernel(const float* planes, const float* pi, const uint8_t* mask,
                                                                          const m0_rowpack_pos* pos, const int64_t* pi_off,
                                                                          const int64_t* mask_off, const int32_t* raw_slot, int n,
                                                                          uint16_t* pi_idx, float* pi_val, uint16_t* mask_idx,
                                                                          float* raw_planes, float* raw_pi, uint8_t* raw_mask) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (row >= n) return;
    const int rk = pos[row].row_kind, mk = pos[row].mask_kind;
    if (rk == M0_ROWPACK_RAW) {
        const size_t slot = (size_t)raw_slot[row];
        copy_pieces(raw_planes + slot * PLANE_FLOATS, planes + (size_t)row * PLANE_FLOATS, PLANE_PIECES, lane);
        if (pi) copy_pieces(raw_pi + slot * COLS, pi + (size_t)row * COLS, PI_PIECES, lane);
        else for (int p = lane; p < PI_PIECES; p += LANES) ((uint4*)(raw_pi + slot * COLS))[p] = make_uint4(0u, 0u, 0u, 0u);
        if (mask) copy_pieces(raw_mask + slot * COLS, mask + (size_t)row * COLS, MASK_PIECES, lane);
        return;
    }
    const float* prow = pi ? pi + (size_t)row * COLS : nullptr;
    int64_t base = pi_off[row];
    for (int k = 0; prow && k < PI_SWEEPS; ++k) {
        const int piece = k * LANES + lane;
        const uint4 v = load_piece(prow, piece, PI_PIECES);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        const int bits = pi_piece_bits(v.x, v.y, v.z, v.w);
        uint64_t ballot[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) ballot[j] = __ballot(bits >> j & 1);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (bits >> j & 1) {
                const int64_t at = base + pi_slot(ballot, bits, lane, j);
                pi_idx[at] = (uint16_t)(piece * 4 + j);
                pi_val[at] = __uint_as_float(w[j]);
            }
        base += __popcll(ballot[0]) + __popcll(ballot[1]) + __popcll(ballot[2]) + __popcll(ballot[3]);
    }
    if (mk != M0_ROWPACK_MASK_LIST) return;
    const uint8_t* mrow = mask + (size_t)row * COLS;
    int64_t mbase = mask_off[row];
    for (int k = 0; k < MASK_SWEEPS; ++k) {
        const int piece = k * LANES + lane;
        const uint4 v = load_piece(mrow, piece, MASK_PIECES);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        bool other = false;                                                                // the count pass made such a row RAW
        int bits = mask_piece_bits(w, other), total;
        int64_t at = mbase + wave_prefix(__popc(bits), lane, total);
        while (bits) {
            const int j = __ffs(bits) - 1;
            bits &= bits - 1;
            mask_idx[at++] = (uint16_t)(piece * 16 + j);
        }
        mbase += total;
    }
}

// One dense row of PER-column pieces (PER = 4: floats of pi, PER = 16: bytes of a mask that are 0 or 1) from its entries
// [e, end).  `chunk` holds entry cb + lane of the wave's current 64 entries (column 65535 past the end: above every sweep).
template <int PER, int PIECES>
__device__ __forceinline__ void expand_row(const uint16_t* idx, const float* val, int64_t e, const int64_t end, void* out, int lane) {
    constexpr int SWEEPS = (PIECES + LANES - 1) / LANES;
    int64_t cb = e;
    int ci = cb + lane < end ? (int)idx[cb + lane] : 65535;
    int cv = PER == 4 && cb + lane < end ? (int)__float_as_uint(val[cb + lane]) : 0;
    for (int k = 0; k < SWEEPS; ++k) {
        const int hi = (k + 1) * LANES * PER;
        uint32_t o[4] = {0u, 0u, 0u, 0u};
        while (e < end) {                                                                  // uniform: e, end, cb and c are
            if (e - cb >= LANES) {
                cb += LANES;
                ci = cb + lane < end ? (int)idx[cb + lane] : 65535;
                if (PER == 4) cv = cb + lane < end ? (int)__float_as_uint(val[cb + lane]) : 0;
            }
            const int j = (int)(e - cb);
            const int c = lane_value(ci, j);
            if (c >= hi) break;
            const bool mine = entry_lane(c, PER) == lane;
            if (PER == 4) {
                const uint32_t v = (uint32_t)lane_value(cv, j);
#pragma unroll
                for (int t = 0; t < 4; ++t) o[t] = mine && (c & 3) == t ? v : o[t];
            } else {
#pragma unroll
                for (int t = 0; t < 4; ++t) o[t] |= mine && ((c & 15) >> 2) == t ? 1u << ((c & 3) * 8) : 0u;
            }
            ++e;
        }
        const int piece = k * LANES + lane;
        if (piece < PIECES) ((uint4*)out)[piece] = make_uint4(o[0], o[1], o[2], o[3]);
    }
}

__global__ __launch_bounds__(64 * ROWS_PER_BLOCK) void rowpack_unpack_kernel(const m0_rowpack_pos* pos, const int64_t* pi_off,
                                                                            const uint16_t* pi_idx, const float* pi_val,
                                                                            const int64_t* mask_off, const uint16_t* mask_idx,
                                                                            const int32_t* raw_slot, const float* raw_planes,
                                                                            const float* raw_pi, const uint8_t* raw_mask, int n,
                                                                            float* planes, float* pi, uint8_t* mask) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (row >= n) return;
    const int rk = pos[row].row_kind, mk = pos[row].mask_kind;
    if (rk == M0_ROWPACK_RAW) {
        const size_t slot = (size_t)raw_slot[row];
        copy_pieces(planes + (size_t)row * PLANE_FLOATS, raw_planes + slot * PLANE_FLOATS, PLANE_PIECES, lane);
        copy_pieces(pi + (size_t)row * COLS, raw_pi + slot * COLS, PI_PIECES, lane);
        if (mask) copy_pieces(mask + (size_t)row * COLS, raw_mask + slot * COLS, MASK_PIECES, lane);
        return;
    }
    expand_row<4, PI_PIECES>(pi_idx, pi_val, pi_off[row], pi_off[row + 1], pi + (size_t)row * COLS, lane);
    if (mask && mk == M0_ROWPACK_MASK_LIST)
        expand_row<16, MASK_PIECES>(mask_idx, nullptr, mask_off[row], mask_off[row + 1], mask + (size_t)row * COLS, lane);
}

}  // namespace

hipError_t launch_rowpack_count(const float* pi, const uint8_t* mask, const Pos* pos, const int32_t* status, int n,
                                m0_rowpack_pos* out_pos, int32_t* counts, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(rowpack_count_kernel, dim3((n + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK), dim3(64 * ROWS_PER_BLOCK), 0, st, pi, mask,
                       pos, status, n, out_pos, counts);
    return hipGetLastError();
}

hipError_t launch_rowpack_fill(const float* planes, const float* pi, const uint8_t* mask, const m0_rowpack_pos* pos,
                               const int64_t* pi_off, const int64_t* mask_off, const int32_t* raw_slot, int n, uint16_t* pi_idx,
                               float* pi_val, uint16_t* mask_idx, float* raw_planes, float* raw_pi, uint8_t* raw_mask, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(rowpack_fill_kernel, dim3((n + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK), dim3(64 * ROWS_PER_BLOCK), 0, st, planes, pi,
                       mask, pos, pi_off, mask_off, raw_slot, n, pi_idx, pi_val, mask_idx, raw_planes, raw_pi, raw_mask);
    return hipGetLastError();
}

hipError_t launch_rowpack_unpack(const m0_rowpack_pos* pos, const int64_t* pi_off, const uint16_t* pi_idx, const float* pi_val,
                                 const int64_t* mask_off, const uint16_t* mask_idx, const int32_t* raw_slot, const float* raw_planes,
                                 const float* raw_pi, const uint8_t* raw_mask, int n, float* planes, float* pi, uint8_t* mask,
                                 hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(rowpack_unpack_kernel, dim3((n + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK), dim3(64 * ROWS_PER_BLOCK), 0, st, pos,
                       pi_off, pi_idx, pi_val, mask_off, mask_idx, raw_slot, raw_planes, raw_pi, raw_mask, n, planes, pi, mask);
    return hipGetLastError();
}
