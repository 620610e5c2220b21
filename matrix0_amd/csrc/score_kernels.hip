// score_rows_kernel: the training loss of stored rows on the device (include/m0_score.h; the arithmetic is score_core.h).
// One wave64 per row, ROWS_PER_WG rows per workgroup.  A lane reads its 16-byte pieces of the row's logits and pi and the four
// mask bytes beside each (piece k * 64 + lane, k = 0..18; 4672 columns are 1168 pieces, so the last sweep covers lanes 0-15)
// ONCE into registers, folds them with Scan::add, the lanes are merged by a fixed shuffle tree (lane i takes lane i + 32, then
// + 16, ... + 1; lane 0 holds the row), the Plan goes back to every lane, and the same registers are folded again with Tail::add
// and merged the same way.  Lane 0 finishes and stores the row's 8 columns as two 16-byte stores.  No atomics, no LDS: a row's
// result is a function of that row alone, whatever B, the row's index or the run.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "score_core.h"
#include "score_kernels.h"

using namespace m0score;

namespace {

constexpr int ROWS_PER_WG = 4;

__device__ __forceinline__ float down(float v, int off) { return __shfl_down(v, off, LANES); }
__device__ __forceinline__ int down(int v, int off) { return __shfl_down(v, off, LANES); }

__device__ __forceinline__ Scan scan_from(const Scan& s, int off) {
    Scan o;
    o.sup.m = down(s.sup.m, off); o.sup.s = down(s.sup.s, off); o.all.m = down(s.all.m, off); o.all.s = down(s.all.s, off);
    o.n = down(s.n, off); o.nq = down(s.nq, off); o.ps = down(s.ps, off); o.a = down(s.a, off); o.u = down(s.u, off);
    o.p_all = down(s.p_all, off); o.poison = down(s.poison, off);
    o.best_pi = down(s.best_pi, off); o.best_logit = down(s.best_logit, off); o.best_idx = down(s.best_idx, off);
    return o;
}

__global__ __launch_bounds__(ROWS_PER_WG * LANES) void score_rows_kernel(const float* __restrict__ logits, const float* __restrict__ value,
                                                                        const float* __restrict__ pi, const float* __restrict__ z,
                                                                        const uint8_t* __restrict__ legal_mask, int B,
                                                                        m0_score_opts opts, float* __restrict__ rows) {
    const int lane = threadIdx.x % LANES;
    const int row = blockIdx.x * ROWS_PER_WG + threadIdx.x / LANES;
    if (row >= B) return;                                   // the whole wave: nothing below synchronises across waves
    const bool masked = opts.mask_mode == M0_SCORE_MASK_LEGAL;
    const float4* lrow = reinterpret_cast<const float4*>(logits + (size_t)row * COLS);
    const float4* prow = reinterpret_cast<const float4*>(pi + (size_t)row * COLS);
    const uint32_t* mrow = reinterpret_cast<const uint32_t*>(legal_mask + (size_t)row * COLS);

    float4 lg[SWEEPS], pv[SWEEPS];
    uint32_t mk[SWEEPS];
#pragma unroll
    for (int k = 0; k < SWEEPS; ++k) {
        const int piece = k * LANES + lane;
        const bool in = piece < F4;
        lg[k] = in ? lrow[piece] : make_float4(0.f, 0.f, 0.f, 0.f);
        pv[k] = in ? prow[piece] : make_float4(0.f, 0.f, 0.f, 0.f);
        mk[k] = (in && masked) ? mrow[piece] : 0u;
    }

    Scan scan;
    scan.mode = opts.mask_mode;
#pragma unroll
    for (int k = 0; k < SWEEPS; ++k) {
        const int piece = k * LANES + lane;
        if (piece < F4) {
            const int col = piece * 4;
            scan.add(col + 0, lg[k].x, pv[k].x, (mk[k] & 0x000000ffu) != 0);
            scan.add(col + 1, lg[k].y, pv[k].y, (mk[k] & 0x0000ff00u) != 0);
            scan.add(col + 2, lg[k].z, pv[k].z, (mk[k] & 0x00ff0000u) != 0);
            scan.add(col + 3, lg[k].w, pv[k].w, (mk[k] & 0xff000000u) != 0);
        }
    }
#pragma unroll
    for (int off = LANES / 2; off > 0; off >>= 1) {
        const Scan o = scan_from(scan, off);
        if (lane < off) scan.merge(o);
    }

    // lane 0 holds the row's scan; every lane needs the plan made from it
    Plan plan(opts, scan);
    plan.uniform = __shfl((int)plan.uniform, 0, LANES) != 0;
    plan.target_logit = __shfl(plan.target_logit, 0, LANES);
    plan.c = __shfl(plan.c, 0, LANES);

    Tail tail;
#pragma unroll
    for (int k = 0; k < SWEEPS; ++k) {
        if (k * LANES + lane < F4) {
            tail.add(plan, lg[k].x, pv[k].x, (mk[k] & 0x000000ffu) != 0);
            tail.add(plan, lg[k].y, pv[k].y, (mk[k] & 0x0000ff00u) != 0);
            tail.add(plan, lg[k].z, pv[k].z, (mk[k] & 0x00ff0000u) != 0);
            tail.add(plan, lg[k].w, pv[k].w, (mk[k] & 0xff000000u) != 0);
        }
    }
#pragma unroll
    for (int off = LANES / 2; off > 0; off >>= 1) {
        Tail o;
        o.rank = down(tail.rank, off);
        o.npos = down(tail.npos, off);
        o.h = down(tail.h, off);
        if (lane < off) tail.merge(o);
    }

    if (lane == 0) {
        float out[M0_SCORE_COLS];
        finish(opts, scan, plan, tail, value[row], z[row], out);
        float4* dst = reinterpret_cast<float4*>(rows + (size_t)row * M0_SCORE_COLS);
        dst[0] = make_float4(out[0], out[1], out[2], out[3]);
        dst[1] = make_float4(out[4], out[5], out[6], out[7]);
    }
}

}  // namespace

hipError_t launch_score_rows(const float* logits, const float* value, const float* pi, const float* z, const uint8_t* legal_mask,
                             int B, const m0_score_opts& opts, float* rows, hipStream_t stream) {
    const int grid = (B + ROWS_PER_WG - 1) / ROWS_PER_WG;
    score_rows_kernel<<<grid, ROWS_PER_WG * LANES, 0, stream>>>(logits, value, pi, z, legal_mask, B, opts, rows);
    return hipGetLastError();
}
