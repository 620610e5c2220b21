/* Training loss of stored positions, read-only: how well a network fits rows (s, pi, z, legal_mask) of the shard store, as the
 * reference's trainer measures it (azchess/training/train.py:436-549) but per row and without a trainer (m0_engine.h includes
 * this file: the calls here are part of the same C ABI and the same library).  No gradient, no WDL term; the SSL term is
 * m0_ssl_score.h, the trainer's flip and rotate augmentations are m0_augment.h (m0_net_score_aug).
 *
 * Per row, with pi >= 0 (4672 columns) and the network's logits and value v:
 *   support   M0_SCORE_MASK_LEGAL: legal_mask | (pi > 0)  (:444-449); _TARGET: pi > 0 (apply_policy_mask, :82); _NONE: every
 *             column (:460).  Columns outside it contribute nothing (the reference fills them with -1e9; their pi is 0).
 *   zero-sum  under _LEGAL a row whose pi sums to <= 0 takes pi = uniform over its legal moves (:210-217; there for the whole
 *             batch as soon as one row needs it, here for that row alone) and carries flag 4.
 *   policy    -sum(pi_s * log_softmax(logits over the support)), pi_s = (1 - eps) * pi + eps * q / |q|, eps = label_smoothing;
 *             q is the support, except under _NONE, where the reference smooths over pi > 0 (:508-512).
 *   value     (v - z)^2, or smooth_l1(v, z, beta = huber_delta) as torch defines it (:546-549).
 * Columns of a row (floats):
 *   0 policy loss   1 entropy of pi_s (0 log 0 = 0; KL = col 0 - col 1)   2 value loss
 *   3 rank of the target's best move: support columns whose logit is strictly greater than the logit at argmax(pi), the lowest
 *     index among equal pi (under flag 4: the lowest legal index); 0 is a top-1 hit, equal logits count as hits
 *   4 mass of the UNMASKED soft-max on the support (1 - illegal_prob_mass of :476-478)
 *   5 size of the support   6 v (0 when it is not finite, :536-538)
 *   7 flags, an integer-valued float: 1 empty support, 2 a non-finite logit among the 4672 or a non-finite v, 4 uniform fallback.
 * A row with flag 1 or 2 has columns 0-4 zero.  A row's result depends on that row alone: the same bits for any B, any row
 * index and any repetition. */
#ifndef M0_SCORE_H
#define M0_SCORE_H
#ifdef __cplusplus
extern "C" {
#endif

#define M0_SCORE_MASK_LEGAL 0
#define M0_SCORE_MASK_TARGET 1
#define M0_SCORE_MASK_NONE 2
#define M0_SCORE_COLS 8
#define M0_SCORE_FLAG_EMPTY 1
#define M0_SCORE_FLAG_NONFINITE 2
#define M0_SCORE_FLAG_UNIFORM 4

typedef struct m0_score_opts {
    int mask_mode;         /* M0_SCORE_MASK_* */
    float label_smoothing; /* [0, 1) */
    int value_loss;        /* 0 mse, 1 huber */
    float huber_delta;     /* > 0 */
} m0_score_opts;

/* The kernel alone, on host arrays: logits [B][4672], value [B], pi [B][4672], z [B], legal_mask [B][4672] u8 (required under
 * M0_SCORE_MASK_LEGAL, otherwise ignored and nullable) -> rows [B][M0_SCORE_COLS].  Non-finite inputs only set flag 2.
 * M0_ERR_INVALID, with `rows` untouched: a null pointer, B <= 0, mask_mode out of range, M0_SCORE_MASK_LEGAL without a mask,
 * label_smoothing outside [0, 1), huber_delta <= 0. */
int m0_score_rows(int hip_device, const float* logits, const float* value, const float* pi, const float* z,
                  const uint8_t* legal_mask, int B, const m0_score_opts* opts, float* rows);
/* Forward and score: planes [B][P][8][8] as m0_net_infer takes them; the logits never leave the device.  The same argument
 * checks.  M0_ERR_NONFINITE when a row carries flag 2, as m0_net_infer answers such outputs; `rows` is written all the same. */
int m0_net_score(m0_net* net, const float* planes, const float* pi, const float* z, const uint8_t* legal_mask, int B,
                 const m0_score_opts* opts, float* rows);
/* score_rows_kernel alone on resident synthetic inputs of B rows (with a mask, M0_SCORE_MASK_LEGAL), `iters` launches between
 * two events after one warm-up: *us_per_launch, and *bytes_per_launch = the bytes a launch must move (tools/bench_score.py). */
int m0_score_bench(int hip_device, int B, int iters, float* us_per_launch, double* bytes_per_launch);

#ifdef __cplusplus
}
#endif
#endif /* M0_SCORE_H */
