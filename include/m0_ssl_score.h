/* The SSL part of the training loss of stored positions, read-only: how well a network's SSL heads fit rows of the shard store,
 * as the reference's trainer measures it (PolicyValueNet.get_enhanced_ssl_loss, azchess/model/resnet.py:892-1130, called from
 * training/train.py:551-677) but per row and without a trainer (m0_engine.h includes this file: the calls here are part of the
 * same C ABI and the same library).  The counterpart of m0_score.h for the term `ssl_weight * ssl_loss`.  No gradient, no WDL.
 *
 * A row has 64 squares (tensor order, row 0 = rank 8).  Its targets are the reference's maps (ssl_algorithms.py:519-543), either
 * as stored with the row, f32 [17][64] in the layout of m0_game_record.ssl (piece one-hot 13, threat, pin, fork, control), or
 * taken from the row's stored planes: they need only planes 0-11 (the pieces) and plane 12 (the side to move) of encode_board.
 * A row of planes is USABLE for that when every value of planes 0-11 is 0 or 1, no square has two pieces, and plane 12 is one
 * value over the board, 0 or 1; nothing else is checked.
 *
 * Per square, in fp32, for the tasks of a bitmask of M0_SSL_* (head channels in the order piece 13, threat 1, pin 1, fork 1,
 * control 3, f32 [C][64] per row as the forward leaves them):
 *   piece     cross-entropy of the 13 logits against the arg-max of the 13 target channels (the first maximum)
 *   threat, pin, fork   max(z, 0) - z t + log(1 + exp(-|z|)), t clamped to [0, 1]
 *   control   cross-entropy of the 3 logits against class 0 / 1 / 2 for a target < -0.5 / otherwise / > 0.5
 * Columns of a row (floats):
 *   0-4   loss of piece, threat, pin, fork, control: the mean over the row's 64 squares; 0 for a task that is not asked for.  The
 *         mean of a column over rows is the reference's batch mean over positions x squares.
 *   5     squares where the arg-max of the piece logits (the lowest index among equals) is the target class
 *   6, 7  the same count over occupied squares only (target class not "empty"); the number of occupied squares
 *   8-10  threat: squares with logit > 0 and target >= 0.5; with logit > 0; with target >= 0.5
 *   11-13 the same three for fork
 *   14    squares where the arg-max of the control logits is the target class
 *   15    flags, an integer-valued float: 1 the planes are not usable (the row then has no targets unless they were given);
 *         2 a non-finite head output in a task asked for; 4 targets were given, the planes are usable, and on some square the two
 *         fall into different classes for a task asked for.
 * A row with flag 2, or with flag 1 and no targets given, has columns 0-14 zero.  A row's result depends on that row alone: the
 * same bits for any B, any row index and any repetition -- and the same bits as the host build of the same arithmetic
 * (csrc/ssl_score_core.h carries its own exp and log). */
#ifndef M0_SSL_SCORE_H
#define M0_SSL_SCORE_H
#ifdef __cplusplus
extern "C" {
#endif

#define M0_SSL_SCORE_COLS 16
#define M0_SSL_SCORE_FLAG_PLANES 1
#define M0_SSL_SCORE_FLAG_NONFINITE 2
#define M0_SSL_SCORE_FLAG_MISMATCH 4

/* The kernel alone, on host arrays: heads [B][C][64] for the C channels of `tasks`, planes [B][19][64], targets [B][17][64] or
 * null (then they are taken from the planes) -> rows [B][M0_SSL_SCORE_COLS].  Non-finite inputs only set flag 2.
 * M0_ERR_INVALID, with `rows` untouched: a null heads, planes or rows, B <= 0, tasks not a non-empty set of M0_SSL_* bits. */
int m0_ssl_score_rows(int hip_device, const float* heads, int tasks, const float* planes, const float* targets, int B,
                      float* rows);
/* One forward with the SSL heads, then both scores on the buffers it left: rows [B][M0_SCORE_COLS] exactly as m0_net_score
 * writes them, ssl_rows [B][M0_SSL_SCORE_COLS] for the network's own tasks; ssl_targets [B][17][64] or null.  Neither the logits
 * nor the head outputs leave the device.  M0_ERR_INVALID for a network without SSL heads, a null ssl_rows and everything
 * m0_net_score refuses, with both outputs untouched.  M0_ERR_NONFINITE when a row of either output carries its non-finite
 * flag; both are written all the same. */
int m0_net_score_ssl(m0_net* net, const float* planes, const float* pi, const float* z, const uint8_t* legal_mask,
                     const float* ssl_targets, int B, const m0_score_opts* opts, float* rows, float* ssl_rows);
/* The targets of stored planes [n][19][64] -> out [n][17][64], the layout of m0_ssl_targets_fens; status [n]: 0, or 1 for a row
 * that is not usable, whose 17 maps in `out` stay as they were.  M0_ERR_INVALID for a null pointer or n <= 0. */
int m0_ssl_targets_planes(int hip_device, const float* planes, int n, float* out, int32_t* status);
/* ssl_score_kernel alone on resident synthetic inputs of B rows, targets from the planes (from_planes != 0) or stored, `iters`
 * launches between two events after one warm-up: *us_per_launch, and *bytes_per_launch = the bytes a launch must move: per row
 * the C head channels and planes 0-12 (256 bytes each), with stored targets their 17 maps as well, and 64 bytes out
 * (tools/bench_ssl_score.py). */
int m0_ssl_score_bench(int hip_device, int B, int tasks, int from_planes, int iters, float* us_per_launch, double* bytes_per_launch);

#ifdef __cplusplus
}
#endif
#endif /* M0_SSL_SCORE_H */
