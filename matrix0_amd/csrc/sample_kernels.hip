// The weights of a resident row store on the device (include/m0_batch_weighted.h; the per-row rules are sample_core.h): written,
// summed per block of BLOCK_ROWS rows, and drawn from.  Every sum is an unsigned 64-bit sum of ticks, so the reduction trees
// and the integer atomics here give the numbers a serial loop gives; there is no float sum and no float atomic anywhere.
//
//   rewrite_blocks_kernel  one workgroup of 256 per block: each row's weight filled or scaled, the block's sum stored afresh.
//   set_weights_kernel     one thread per (id, value): the sanitised value is swapped in (atomicExch, so that of two values for
//                          one id each sees what the other left) and the block's sum moves by ticks(new) - ticks(old) with one
//                          64-bit atomicAdd; the differences telescope, whatever the order.
//   score_weights_kernel   one thread per scored row of a batch (m0_net_score_resident): the rule's weight of the row's score
//                          columns, stored at the row its reference names as set_weights_kernel stores a value.
//   block_prefix_kernel    one workgroup of 1024: the inclusive prefix of all block sums, 1024 blocks a pass.  A draw never
//                          rescans the window, only these sums (one per 1024 rows).
//   draw_kernel            one wave per draw: binary search of r in the prefix, then the block's rows 64 at a time -- coalesced
//                          loads, ticks, an inclusive wave scan in u64 (__shfl_up), a ballot for the first lane past r.  No LDS.
//
// Bounds.  The table holds nseg > 0 resident segments in ascending, contiguous ids; it is rewritten only while nothing enqueued
// through the store is running.  An id is used only after first <= id < first + rows of the table has been checked
// (set_weights_kernel skips and counts the others), so segment_of returns s < nseg and row = id - table[s].first < rows.  A block
// index k is below nb = the blocks of the table: segment_of_block returns s < nseg with 0 <= j = k - block0 < blocks, and a row
// of the block is used only below min(BLOCK_ROWS, rows - j * BLOCK_ROWS).  In a draw r < total = pre[nb], so block_of ends at a
// block k < nb with pre[k] <= r < pre[k + 1]; total == 0 takes the uniform rule, id = first + umulhi64(x, rows) < first + rows.
// Should a block's sum disagree with its rows (weights written on another stream under the draw, which the ordering contract
// leaves to the caller) the scan may run out: the draw then names the block's last row.  So {seg, row} of a row reference always
// names a row of a resident segment, and ids_out, prob_out and refs are written at b < B only.
#include <hip/hip_runtime.h>
#include "sample_core.h"
#include "sample_kernels.h"

using namespace m0sample;
using m0batch::RowRef;

namespace {

constexpr int WAVE = 64;
constexpr int REWRITE_THREADS = 256;
constexpr int PREFIX_THREADS = 1024;
constexpr int DRAW_WAVES = 4;

// the segment of block k: the last entry whose first block is not above it.  n > 0, 0 <= k < the blocks of the table.
__device__ int segment_of_block(const SegEntry* table, int n, int k) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].block0 <= k) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ uint64_t wave_inclusive_scan(uint64_t v, int lane) {
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
        const uint64_t up = __shfl_up((unsigned long long)v, d);
        if (lane >= d) v += up;
    }
    return v;
}

__device__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
    for (int d = WAVE / 2; d > 0; d >>= 1) v += __shfl_down((unsigned long long)v, d);
    return v;                                                             // lane 0 holds the sum
}

__global__ __launch_bounds__(REWRITE_THREADS) void rewrite_blocks_kernel(const SegEntry* __restrict__ table, int nseg, int k0, int nk,
                                                                        int mode, int64_t lo, int64_t hi, float value) {
    __shared__ uint64_t part[REWRITE_THREADS / WAVE];
    const int k = k0 + (int)blockIdx.x, t = threadIdx.x;
    if ((int)blockIdx.x >= nk) return;
    const SegEntry e = table[segment_of_block(table, nseg, k)];
    const int j = k - e.block0;
    const int64_t base = (int64_t)j * BLOCK_ROWS;
    const int n = (int)(e.rows - base < BLOCK_ROWS ? e.rows - base : BLOCK_ROWS);
    uint64_t sum = 0;
    for (int i = t; i < n; i += REWRITE_THREADS) {
        float w = e.w[base + i];
        if (mode == M0_REWRITE_SCALE) {
            w = scaled(w, value);
            e.w[base + i] = w;
        } else if (e.first + base + i >= lo && e.first + base + i < hi) {
            w = value;
            e.w[base + i] = w;
        }
        sum += ticks(w);
    }
    sum = wave_sum(sum);
    if ((t & (WAVE - 1)) == 0) part[t / WAVE] = sum;
    __syncthreads();
    if (t == 0) {
        uint64_t all = 0;
        for (int i = 0; i < REWRITE_THREADS / WAVE; ++i) all += part[i];
        e.bsum[j] = all;
    }
}

__global__ __launch_bounds__(256) void set_weights_kernel(const SegEntry* __restrict__ table, int nseg, const int64_t* __restrict__ ids,
                                                         const float* __restrict__ values, int64_t n, uint64_t* __restrict__ counters) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool counted = false;
    if (i < n) {
        const int64_t id = ids[i];
        const int64_t first = table[0].first, end = table[nseg - 1].first + table[nseg - 1].rows;
        counted = true;                                                   // an id outside the window: skipped
        if (id >= first && id < end) {
            const SegEntry e = table[segment_of(table, nseg, id)];
            const int64_t row = id - e.first;
            if (row >= 0 && row < e.rows) {
                const float w = sanitise(values[i], &counted);
                const float old = atomicExch(&e.w[row], w);
                const uint64_t delta = ticks(w) - ticks(old);             // modulo 2^64: the sum is exact
                if (delta != 0) atomicAdd((unsigned long long*)&e.bsum[row / BLOCK_ROWS], (unsigned long long)delta);
            }
        }
    }
    const unsigned long long votes = __ballot(counted);
    if ((threadIdx.x & (WAVE - 1)) == 0 && votes != 0) atomicAdd((unsigned long long*)counters, (unsigned long long)__popcll(votes));
}

// One thread per scored row: the weight the rule makes of the row's columns goes to the row its reference names, as
// set_weights_kernel stores a value.  refs [B] are those of the batch that was scored: the host has checked row < seg->n, and a
// reference whose segment is not in the table (there is none) is left alone, so w and bsum are indexed inside their segment.
__global__ __launch_bounds__(256) void score_weights_kernel(const SegEntry* __restrict__ table, int nseg, const RowRef* __restrict__ refs,
                                                           const float* __restrict__ score_rows, int B, m0_weight_rule rule) {
    const int b = (int)blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const RowRef ref = refs[b];
    int s = 0;
    while (s < nseg && table[s].view != ref.seg) ++s;
    if (s == nseg || ref.row < 0 || ref.row >= table[s].rows) return;
    const SegEntry e = table[s];
    const float* c = score_rows + (size_t)b * M0_SCORE_COLS;
    const float w = weight_from_score(rule, c[0], c[1], c[2]);
    const float old = atomicExch(&e.w[ref.row], w);
    const uint64_t delta = ticks(w) - ticks(old);
    if (delta != 0) atomicAdd((unsigned long long*)&e.bsum[ref.row / BLOCK_ROWS], (unsigned long long)delta);
}

__global__ __launch_bounds__(PREFIX_THREADS) void block_prefix_kernel(const SegEntry* __restrict__ table, int nseg, int nb,
                                                                     uint64_t* __restrict__ pre) {
    __shared__ uint64_t wave_total[PREFIX_THREADS / WAVE];
    const int t = threadIdx.x, lane = t & (WAVE - 1), wave = t / WAVE;
    uint64_t carry = 0;                                                   // the ticks of the blocks of earlier passes, in every thread
    if (t == 0) pre[0] = 0;
    for (int k0 = 0; k0 < nb; k0 += PREFIX_THREADS) {
        const int k = k0 + t;
        uint64_t v = 0;
        if (k < nb) {
            const SegEntry& e = table[segment_of_block(table, nseg, k)];
            v = e.bsum[k - e.block0];
        }
        v = wave_inclusive_scan(v, lane);
        if (lane == WAVE - 1) wave_total[wave] = v;
        __syncthreads();
        uint64_t before = carry, pass = 0;
        for (int i = 0; i < PREFIX_THREADS / WAVE; ++i) {
            if (i < wave) before += wave_total[i];
            pass += wave_total[i];
        }
        if (k < nb) pre[k + 1] = before + v;
        carry += pass;
        __syncthreads();
    }
}

__global__ __launch_bounds__(DRAW_WAVES * WAVE) void draw_kernel(const SegEntry* __restrict__ table, int nseg, int nb,
                                                                const uint64_t* __restrict__ pre, int B, uint64_t seed, uint64_t draw,
                                                                int stratified, int64_t* __restrict__ ids_out, float* __restrict__ prob_out,
                                                                RowRef* __restrict__ refs, uint64_t* __restrict__ counters) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int b = (int)blockIdx.x * DRAW_WAVES + __builtin_amdgcn_readfirstlane((int)threadIdx.x / WAVE);
    if (b >= B) return;                                                   // the whole wave
    const uint64_t total = pre[nb];
    const uint64_t x = draw_x(draw_key(seed, draw), b);
    int s;
    int64_t row;
    float prob;
    if (total == 0) {
        const int64_t first = table[0].first, rows = table[nseg - 1].first + table[nseg - 1].rows - first;
        const int64_t id = first + uniform_offset(x, rows);
        s = segment_of(table, nseg, id);
        row = id - table[s].first;
        prob = uniform_prob(rows);
        if (b == 0 && lane == 0) atomicAdd((unsigned long long*)(counters + 1), 1ull);
    } else {
        const uint64_t r = draw_r(x, b, B, stratified != 0, total);
        const int k = block_of(pre, nb, r);
        s = segment_of_block(table, nseg, k);
        const SegEntry e = table[s];
        const int64_t base = (int64_t)(k - e.block0) * BLOCK_ROWS;
        const int n = (int)(e.rows - base < BLOCK_ROWS ? e.rows - base : BLOCK_ROWS);
        const float* w = e.w + base;
        uint64_t left = r - pre[k];
        int at = -1;
        uint64_t at_ticks = 0;
        for (int c = 0; c < n; c += WAVE) {
            const uint64_t t = c + lane < n ? ticks(w[c + lane]) : 0;
            const uint64_t incl = wave_inclusive_scan(t, lane);
            const uint64_t sum = __shfl((unsigned long long)incl, WAVE - 1);
            if (left < sum) {
                const int l = __ffsll((unsigned long long)__ballot(incl > left)) - 1;
                at = c + l;
                at_ticks = __shfl((unsigned long long)t, l);
                break;
            }
            left -= sum;
        }
        if (at < 0) { at = n - 1; at_ticks = ticks(w[at]); }               // the block's sum was not that of its rows (see above)
        row = base + at;
        prob = draw_prob(at_ticks, total);
    }
    if (lane == 0) {
        ids_out[b] = table[s].first + row;
        prob_out[b] = prob;
        if (refs) { refs[b].seg = table[s].view; refs[b].row = (int32_t)row; }
    }
}

}  // namespace

hipError_t launch_rewrite_blocks(const SegEntry* table, int nseg, int k0, int nk, int mode, int64_t lo, int64_t hi, float value,
                                 hipStream_t st) {
    if (!table || nseg <= 0 || k0 < 0 || nk <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rewrite_blocks_kernel, dim3(nk), dim3(REWRITE_THREADS), 0, st, table, nseg, k0, nk, mode, lo, hi, value);
    return hipGetLastError();
}

hipError_t launch_set_weights(const SegEntry* table, int nseg, const int64_t* ids, const float* values, int64_t n, uint64_t* counters,
                              hipStream_t st) {
    if (!table || nseg <= 0 || !ids || !values || !counters || n <= 0 || n > (int64_t)1 << 38) return hipErrorInvalidValue;
    hipLaunchKernelGGL(set_weights_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, table, nseg, ids, values, n, counters);
    return hipGetLastError();
}

hipError_t launch_score_weights(const SegEntry* table, int nseg, const RowRef* refs, const float* score_rows, int B,
                                const m0_weight_rule& rule, hipStream_t st) {
    if (!table || nseg <= 0 || !refs || !score_rows || B <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(score_weights_kernel, dim3((B + 255) / 256), dim3(256), 0, st, table, nseg, refs, score_rows, B, rule);
    return hipGetLastError();
}

hipError_t launch_draw(const SegEntry* table, int nseg, int nb, uint64_t* pre, int B, uint64_t seed, uint64_t draw, int stratified,
                       int64_t* ids_out, float* prob_out, RowRef* refs, uint64_t* counters, hipStream_t st) {
    if (!table || nseg <= 0 || nb <= 0 || !pre || B <= 0 || !ids_out || !prob_out || !counters) return hipErrorInvalidValue;
    hipLaunchKernelGGL(block_prefix_kernel, dim3(1), dim3(PREFIX_THREADS), 0, st, table, nseg, nb, pre);
    hipLaunchKernelGGL(draw_kernel, dim3((B + DRAW_WAVES - 1) / DRAW_WAVES), dim3(DRAW_WAVES * WAVE), 0, st, table, nseg, nb, pre, B,
                       seed, draw, stratified, ids_out, prob_out, refs, counters);
    return hipGetLastError();
}
