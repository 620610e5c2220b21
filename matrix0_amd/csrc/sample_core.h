// Per-row rules of the weighted row store (include/m0_batch_weighted.h), host and device: sample_kernels.hip runs them one wave per
// draw, sample_host.h runs them on the CPU with plain loops (the host store).  Everything a result depends on is decided here,
// once: the ticks of a weight, what a weight from device memory is sanitised to, the random number of a draw and the probability
// it reports.  All sums are unsigned 64-bit sums of ticks, so no order of summation can change a result.
#pragma once
#include <stdint.h>
#include "../../include/m0_engine.h"
#include "batch_core.h"
#include "chess_core.h"

namespace m0sample {

using m0::mix64;
using m0batch::SegView;

constexpr float WEIGHT_MAX = (float)M0_WEIGHT_MAX;
constexpr float TICK_SCALE = (float)M0_WEIGHT_ONE_TICKS;
// rows whose ticks are summed into one block sum; blocks are counted from a segment's first row, the last one may be short
constexpr int BLOCK_ROWS = 1024;
constexpr uint64_t GOLDEN = 0x9E3779B97F4A7C15ull;
constexpr uint64_t DRAW_MUL = 0xD6E8FEB86659FD93ull;

// One resident segment as the weighted kernels see it; the table of them is in ascending id, ids are contiguous over it.
struct SegEntry {
    int64_t first;                  // id of its first row
    int64_t rows;
    const SegView* view;            // what a row reference names
    float* w;                       // [rows]
    uint64_t* bsum;                 // [blocks]: ticks of rows [j * BLOCK_ROWS, min(rows, (j + 1) * BLOCK_ROWS))
    int32_t block0;                 // index of its first block among the blocks of all segments
    int32_t blocks;
};

M0_HD int blocks_of(int64_t rows) { return (int)((rows + BLOCK_ROWS - 1) / BLOCK_ROWS); }
// a weight a host caller may set: finite, 0 <= w <= WEIGHT_MAX (false for NaN)
M0_HD bool valid_weight(float w) { return w >= 0.f && w <= WEIGHT_MAX; }
// a weight from device memory: NaN or negative -> 0, above the maximum (+inf too) -> the maximum; *changed says whether
M0_HD float sanitise(float w, bool* changed) {
    *changed = !valid_weight(w);
    return w > WEIGHT_MAX ? WEIGHT_MAX : (w >= 0.f ? w : 0.f);
}
// of a valid weight: an exact scaling by 2^24, truncated; at most 2^40
M0_HD uint64_t ticks(float w) { return (uint64_t)(w * TICK_SCALE); }
M0_HD float scaled(float w, float factor) {
    const float v = w * factor;
    return v < WEIGHT_MAX ? v : WEIGHT_MAX;
}

// nullptr for a rule a weight can be made by, otherwise why not
inline const char* bad_rule(const m0_weight_rule* r) {
    if (!r) return "rule is null";
    const float f[5] = {r->policy, r->kl, r->value, r->floor, r->cap};
    for (float v : f)
        if (!(v - v == 0.f)) return "every field of a weight rule must be finite";
    if (r->floor < 0.f) return "floor must not be negative";
    if (r->cap < 0.f || r->cap > WEIGHT_MAX) return "cap must lie in [0, 65536]";
    return nullptr;
}
// the weight of a row with policy loss c0, target entropy c1 and value loss c2: always a valid weight
M0_HD float weight_from_score(const m0_weight_rule& r, float c0, float c1, float c2) {
    float t = r.floor;
    t = fmaf(r.policy, c0, t);
    t = fmaf(r.kl, c0 - c1, t);
    t = fmaf(r.value, c2, t);
    t = t > 0.f ? t : 0.f;                                                // also for a t that is not a number
    return t < r.cap ? t : r.cap;
}

M0_HD uint64_t umulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

M0_HD uint64_t draw_key(uint64_t seed, uint64_t draw) { return mix64(mix64(seed + GOLDEN) ^ (draw * DRAW_MUL)); }
M0_HD uint64_t draw_x(uint64_t key, int b) { return mix64(key + (uint64_t)(b + 1) * GOLDEN); }
// r_b in [0, total) for total > 0
M0_HD uint64_t draw_r(uint64_t x, int b, int B, bool stratified, uint64_t total) {
    if (stratified) {
        const uint64_t q = total / (uint64_t)B, rem = total % (uint64_t)B, ub = (uint64_t)b;
        const uint64_t span = q + (ub < rem ? 1 : 0);
        if (span != 0) return ub * q + (ub < rem ? ub : rem) + umulhi64(x, span);
    }
    return umulhi64(x, total);
}
M0_HD float draw_prob(uint64_t row_ticks, uint64_t total) { return (float)((double)row_ticks / (double)total); }
// total == 0: uniform over the `rows` resident rows
M0_HD int64_t uniform_offset(uint64_t x, int64_t rows) { return (int64_t)umulhi64(x, (uint64_t)rows); }
M0_HD float uniform_prob(int64_t rows) { return (float)(1.0 / (double)rows); }

// the segment of a resident id: the last entry whose first id is not above it.  n > 0 and table[0].first <= id.
M0_HD int segment_of(const SegEntry* table, int n, int64_t id) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].first <= id) lo = mid; else hi = mid - 1;
    }
    return lo;
}
// pre [nb + 1] with pre[0] = 0 and pre[k + 1] the ticks of blocks 0 .. k: the block of r < pre[nb], the smallest k with
// pre[k + 1] > r
M0_HD int block_of(const uint64_t* pre, int nb, uint64_t r) {
    int lo = 0, hi = nb - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (pre[mid + 1] > r) hi = mid; else lo = mid + 1;
    }
    return lo;
}

}  // namespace m0sample
