// Launchers of sample_kernels.hip: the weights of a resident row store written, summed and drawn from on the device
// (include/m0_batch_weighted.h; the per-row rules are sample_core.h).  `table` [nseg] is the store's segment table in device
// memory, in ascending id; a block index k counts the blocks of all segments in that order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "batch_core.h"
#include "sample_core.h"

// what launch_rewrite_blocks does to a row's weight
enum : int { M0_REWRITE_FILL = 0, M0_REWRITE_SCALE = 1 };

// Blocks k0 .. k0 + nk - 1, one workgroup each: FILL gives rows with lo <= id < hi `value` (a valid weight) and leaves the others;
// SCALE gives every row scaled(w, value).  Each block's sum is then stored afresh from its rows.
hipError_t launch_rewrite_blocks(const m0sample::SegEntry* table, int nseg, int k0, int nk, int mode, int64_t lo, int64_t hi,
                                 float value, hipStream_t st);
// ids i64 [n], values f32 [n] in device memory: every resident id gets its sanitised value, and its block's sum moves by the
// difference of the ticks (integer atomics).  counters u64 [2]: [0] grows by the values sanitised and the ids skipped.
hipError_t launch_set_weights(const m0sample::SegEntry* table, int nseg, const int64_t* ids, const float* values, int64_t n,
                              uint64_t* counters, hipStream_t st);
// refs [B] of a batch in device memory and score_rows f32 [B][M0_SCORE_COLS] of its rows (score_kernels.hip), device memory: row
// refs[b] gets weight_from_score(rule, its columns 0, 1, 2), and its block's sum moves as in launch_set_weights.
hipError_t launch_score_weights(const m0sample::SegEntry* table, int nseg, const m0batch::RowRef* refs, const float* score_rows, int B,
                                const m0_weight_rule& rule, hipStream_t st);
// pre u64 [nb + 1]: pre[0] = 0, pre[k + 1] the ticks of blocks 0 .. k; and behind it B draws, one wave each: ids_out i64 [B],
// prob_out f32 [B] and, when refs is not null, {seg, row} of refs [B] (kind stays as it is).  counters[1] grows by one when the
// total is 0.  nseg > 0, nb the blocks of the table, B > 0.
hipError_t launch_draw(const m0sample::SegEntry* table, int nseg, int nb, uint64_t* pre, int B, uint64_t seed, uint64_t draw,
                       int stratified, int64_t* ids_out, float* prob_out, m0batch::RowRef* refs, uint64_t* counters, hipStream_t st);
