// Host side of the weighted row store (include/m0_batch_weighted.h), plain C++ without HIP: what sample_kernels.hip does, with
// straight loops over sample_core.h on a segment table whose pointers are host memory.  Used by capi_batch_weighted.hip for a
// host store.  The block sums are kept as on the device, so a draw walks the same two levels; the numbers are sums of integers
// and cannot differ.
#pragma once
#include <vector>
#include "sample_core.h"

namespace m0sample {

inline int host_segment_of_block(const SegEntry* table, int n, int k) {
    int s = 0;
    while (s + 1 < n && table[s + 1].block0 <= k) ++s;
    return s;
}

// blocks k0 .. k0 + nk - 1 as rewrite_blocks_kernel rewrites them: fill (scale false) of the ids in [lo, hi), or scale
inline void host_rewrite_blocks(const SegEntry* table, int nseg, int k0, int nk, bool scale, int64_t lo, int64_t hi, float value) {
    for (int k = k0; k < k0 + nk; ++k) {
        const SegEntry& e = table[host_segment_of_block(table, nseg, k)];
        const int j = k - e.block0;
        const int64_t base = (int64_t)j * BLOCK_ROWS;
        const int64_t n = e.rows - base < BLOCK_ROWS ? e.rows - base : BLOCK_ROWS;
        uint64_t sum = 0;
        for (int64_t i = 0; i < n; ++i) {
            float& w = e.w[base + i];
            if (scale) w = scaled(w, value);
            else if (e.first + base + i >= lo && e.first + base + i < hi) w = value;
            sum += ticks(w);
        }
        e.bsum[j] = sum;
    }
}

// resident ids and valid weights (the caller has checked both)
inline void host_set_weights(const SegEntry* table, int nseg, const int64_t* ids, const float* values, int64_t n) {
    for (int64_t i = 0; i < n; ++i) {
        const SegEntry& e = table[segment_of(table, nseg, ids[i])];
        const int64_t row = ids[i] - e.first;
        e.bsum[row / BLOCK_ROWS] += ticks(values[i]) - ticks(e.w[row]);
        e.w[row] = values[i];
    }
}

// pre [nb + 1] as block_prefix_kernel writes it
inline void host_block_prefix(const SegEntry* table, int nseg, int nb, uint64_t* pre) {
    pre[0] = 0;
    for (int s = 0; s < nseg; ++s)
        for (int j = 0; j < table[s].blocks; ++j) pre[table[s].block0 + j + 1] = pre[table[s].block0 + j] + table[s].bsum[j];
    (void)nb;
}

// B draws as draw_kernel makes them; refs, when not null, get {seg, row}.  True when the total was 0 (the uniform rule).
inline bool host_draw(const SegEntry* table, int nseg, int nb, const uint64_t* pre, int B, uint64_t seed, uint64_t draw, bool stratified,
                      int64_t* ids_out, float* prob_out, m0batch::RowRef* refs) {
    const uint64_t total = pre[nb], key = draw_key(seed, draw);
    for (int b = 0; b < B; ++b) {
        const uint64_t x = draw_x(key, b);
        int s;
        int64_t row;
        if (total == 0) {
            const int64_t first = table[0].first, rows = table[nseg - 1].first + table[nseg - 1].rows - first;
            const int64_t id = first + uniform_offset(x, rows);
            s = segment_of(table, nseg, id);
            row = id - table[s].first;
            prob_out[b] = uniform_prob(rows);
        } else {
            const uint64_t r = draw_r(x, b, B, stratified, total);
            const int k = block_of(pre, nb, r);
            s = host_segment_of_block(table, nseg, k);
            const SegEntry& e = table[s];
            const int64_t base = (int64_t)(k - e.block0) * BLOCK_ROWS;
            const int64_t n = e.rows - base < BLOCK_ROWS ? e.rows - base : BLOCK_ROWS;
            uint64_t run = pre[k];
            int64_t at = n - 1;
            for (int64_t i = 0; i < n; ++i) {
                run += ticks(e.w[base + i]);
                if (run > r) { at = i; break; }
            }
            row = base + at;
            prob_out[b] = draw_prob(ticks(e.w[row]), total);
        }
        ids_out[b] = table[s].first + row;
        if (refs) { refs[b].seg = table[s].view; refs[b].row = (int32_t)row; }
    }
    return total == 0;
}

}  // namespace m0sample
