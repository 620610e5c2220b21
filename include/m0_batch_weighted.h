/* A weight per resident row of a row store, and batches drawn in proportion to it on the device (m0_engine.h includes this file
 * behind m0_batch_ssl.h: the calls here are part of the same C ABI and the same library).  m0_rowstore_batch turns row ids into a
 * batch; which ids go into it was the host's choice, and a uniform one.  With the calls here a store is a prioritised replay
 * buffer: weights are written, drawn from and gathered behind each other on one stream without a host synchronisation between.
 *
 *   weights   one float per resident row, finite, 0 <= w <= M0_WEIGHT_MAX.  They are allocated at the first call of this header
 *             on a store; every resident row then has weight 1, and so has every row appended later.  Eviction frees a segment's
 *             weights with the segment.  A store that never sees a call of this header allocates nothing for them, and
 *             m0_rowstore_batch and m0_rowstore_batch_ssl never look at them.  A store with more than M0_WEIGHT_ROWS_MAX resident
 *             rows refuses the calls here (M0_ERR_INVALID).
 *   ticks     ticks(w) = (uint64_t)(w * 16777216.0f): the product is an exact scaling by 2^24, the conversion truncates, a row
 *             has at most 2^40 ticks, a weight below 2^-24 has none and is never drawn.  Every sum is an unsigned 64-bit sum of
 *             ticks and, with at most 2^23 rows, stays below 2^63.  THE FORMAT IS FIXED-POINT SO THAT EVERY RESULT IS EXACT AND
 *             INDEPENDENT OF THE ORDER OF SUMMATION: any reduction tree, any block size and any use of integer atomics give the
 *             same numbers, on the device, in a host store and in a dozen lines of numpy.
 *   the draw  rows in ascending id, S_i the inclusive prefix sum of their ticks, total = S_last.  For r in [0, total) the drawn
 *             row is the smallest id with S_i > r.  With G = 0x9E3779B97F4A7C15, mix64 the finaliser of splitmix64
 *             (x ^= x >> 30, x *= 0xbf58476d1ce4e5b9, x ^= x >> 27, x *= 0x94d049bb133111eb, x ^= x >> 31) and umulhi64 the high
 *             64 bits of a 64 x 64 bit product:
 *                 key = mix64(mix64(seed + G) ^ (draw * 0xD6E8FEB86659FD93))
 *                 x_b = mix64(key + (b + 1) * G)
 *             independent   r_b = umulhi64(x_b, total)
 *             stratified    q = total / B, rem = total % B, span_b = q + (b < rem), lo_b = b * q + min(b, rem),
 *                           r_b = lo_b + umulhi64(x_b, span_b); span_b == 0: the independent rule for that b.  Ids ascend.
 *             prob_b = (float)((double)ticks_i / (double)total).  total == 0: the draw is uniform over the resident rows,
 *             id = first + umulhi64(x_b, rows), prob = 1 / rows, and the launch is counted (degenerate draws) rather than
 *             refused: an enqueued launch cannot refuse.  Output b depends on (seed, draw, b, B, mode, the resident weights) alone.
 *   order     weight writes and draws that must see each other go on ONE stream; otherwise the caller orders them.  Eviction
 *             waits for everything enqueued through the store, as m0_batch.h says.  A draw never names a row outside a resident
 *             segment, whatever the order. */
#ifndef M0_BATCH_WEIGHTED_H
#define M0_BATCH_WEIGHTED_H
#ifdef __cplusplus
extern "C" {
#endif

#define M0_WEIGHT_MAX 65536
/* ticks of weight 1, 2^24 */
#define M0_WEIGHT_ONE_TICKS 16777216
/* resident rows above which a store refuses the calls here, 2^23 */
#define M0_WEIGHT_ROWS_MAX 8388608
/* m0_rowstore_weights_info writes this many int64: the total ticks, the rows with ticks, the values sanitised or skipped by
 * m0_rowstore_set_weights from device memory so far, the launches that drew from a total of 0 so far. */
#define M0_WEIGHTS_INFO 4

/* ids i64 [n], values f32 [n].
 * on_device 0: host arrays (stream is ignored); the call returns with the weights in place.  M0_ERR_INVALID with nothing changed:
 *   an id that is not resident (the message names it), an id that occurs twice, a value that is not a valid weight.
 * on_device 1: device memory of the store's device; the work is enqueued on `stream` and the call does not wait for it.  An id
 *   outside the resident window is skipped and counted.  Values are sanitised: NaN or negative becomes 0, above M0_WEIGHT_MAX
 *   (+inf too) becomes M0_WEIGHT_MAX, each counted.  WHERE AN ID OCCURS MORE THAN ONCE, ONE OF ITS VALUES IS STORED -- which one is
 *   the only unspecified outcome of this header; the sums are exact for the one that was.  Refused for a host store. */
int m0_rowstore_set_weights(m0_rowstore* store, const int64_t* ids, const float* values, int64_t n, int on_device, void* stream);
/* Rows first_id .. first_id + n - 1 (all resident, otherwise M0_ERR_INVALID with nothing changed) get `value`, a valid weight:
 * how new rows get the highest priority.  Returns with the weights in place. */
int m0_rowstore_fill_weights(m0_rowstore* store, int64_t first_id, int64_t n, float value);
/* w = min(M0_WEIGHT_MAX, w * factor), one float multiply, for every resident row; factor finite and not negative.  One call per
 * append gives an exponential decay by age.  Returns with the weights in place. */
int m0_rowstore_scale_weights(m0_rowstore* store, float factor);
/* out_host f32 [n]: the weights of these resident ids (duplicates allowed), after everything enqueued on the device has finished. */
int m0_rowstore_get_weights(m0_rowstore* store, const int64_t* ids, int64_t n, float* out_host);
/* info i64 [M0_WEIGHTS_INFO], after everything enqueued on the device has finished. */
int m0_rowstore_weights_info(m0_rowstore* store, int64_t* info);
/* B draws: ids_out i64 [B], prob_out f32 [B].  outputs_on_device 0: host memory, filled when the call returns; 1: device memory,
 * enqueued on `stream`.  M0_ERR_INVALID: B <= 0, a null output, an empty store, device outputs of a host store. */
int m0_rowstore_sample(m0_rowstore* store, int B, uint64_t seed, uint64_t draw, int stratified, int64_t* ids_out, float* prob_out,
                       int outputs_on_device, void* stream);
/* m0_rowstore_sample and, behind it on `stream`, the batch of the drawn rows: the draw writes the row references on the device and
 * the kernel of m0_rowstore_batch (with ssl and ssl_status: of m0_rowstore_batch_ssl; both NULL: without the maps) consumes them,
 * with no host synchronisation between the two for device outputs.  kinds is the host array of m0_rowstore_batch (u8 [B] or
 * NULL).  The batch is bit for bit what m0_rowstore_batch gives for ids_out and kinds; everything m0_rowstore_batch says about
 * outputs, masks, alignment and allocation holds: after the first call of a size no call allocates or frees. */
int m0_rowstore_batch_sampled(m0_rowstore* store, int B, uint64_t seed, uint64_t draw, int stratified, const uint8_t* kinds,
                              float* planes, float* pi, float* z, uint8_t* mask, float* ssl, int32_t* ssl_status, int64_t* ids_out,
                              float* prob_out, int outputs_on_device, void* stream);

/* How a row's training loss (the columns of m0_score.h: c0 the policy loss, c1 the entropy of its target, c2 the value loss)
 * becomes its weight.  In float32, in exactly this order:
 *     t = floor;  t = fmaf(policy, c0, t);  t = fmaf(kl, c0 - c1, t);  t = fmaf(value, c2, t);  w = min(cap, max(0, t))
 * (a t that is not a number gives 0).  One function for host and device: no pow, no log -- an exponent such as the alpha of
 * prioritised replay stays with the caller, because the device's and the host's pow differ in the last bit.  A flagged row
 * (M0_SCORE_FLAG_EMPTY, _NONFINITE) has zero columns and gets `floor`.  All fields finite, floor >= 0, 0 <= cap <= M0_WEIGHT_MAX;
 * anything else is M0_ERR_INVALID. */
typedef struct m0_weight_rule {
    float policy, kl, value, floor, cap;
} m0_weight_rule;

/* m0_net_score for rows that are resident in a device store: the store's batch kernel fills the network's staging buffers on the
 * network's stream (ids i64 [B] resident, duplicates allowed; kinds u8 [B] or NULL as m0_rowstore_batch takes them), then the
 * forward and the score kernel run as they are; rows_out is the host f32 [B][M0_SCORE_COLS] of m0_net_score, bit for bit what
 * m0_net_score_packed gives for the same rows (with kinds: m0_net_score_aug for the unpacked rows).  rule not NULL: behind the
 * score kernel one more kernel gives every scored row its weight from the device-side columns and brings the block sums up to
 * date -- the loss never crosses to the host for that; where an id occurs twice one of its (equal) weights is stored.  The call
 * returns when all of it has finished.  Locks are taken network first, then store.  M0_ERR_INVALID: a host store, a store on
 * another device than the network's, a store without masks under M0_SCORE_MASK_LEGAL, a network without the 19 planes, an id
 * that is not resident, a rule that is not valid. */
int m0_net_score_resident(m0_net* net, m0_rowstore* store, const int64_t* ids, const uint8_t* kinds, int B, const m0_score_opts* opts,
                          float* rows_out, const m0_weight_rule* rule);
/* The same function on host arrays: rows f32 [B][M0_SCORE_COLS] as a score call returned them -> out f32 [B]. */
int m0_weight_from_score(const float* rows, int B, const m0_weight_rule* rule, float* out);

#ifdef __cplusplus
}
#endif
#endif /* M0_BATCH_WEIGHTED_H */
