/* The trainer's flip and rotate augmentations of stored rows (s, pi, legal_mask), on the device, and the training loss under them
 * (m0_engine.h includes this file: the calls here are part of the same C ABI and the same library).  The reference's trainer
 * (azchess/training/train.py:280-305, augment=True by default) draws one r per batch: r < 0.5 mirrors the files, 0.5 <= r < 0.75
 * rotates by 180 degrees (training.augment_rotate180, default true), otherwise the batch stays as it is.  Here the kind is chosen per
 * row by the caller; matrix0_amd/score.py weighs the three losses as the trainer's draw does.
 *
 * With the policy laid out [rank][file][73] and the planes [P][rank][file], a kind is a map of the squares (M0_AUG_HFLIP: file ->
 * 7 - file; M0_AUG_ROT180: rank -> 7 - rank and file -> 7 - file) and a permutation perm of the 73 move-type channels
 * (build_horizontal_flip_permutation / build_rotate180_permutation, azchess/encoding.py:310-386; csrc/augment_core.h):
 *   s'[p][sq] = s[p][map(sq)]     pi'[sq][c] = pi[map(sq)][perm[c]]     legal_mask' as pi'     z unchanged
 * which is torch.flip followed by index_select(-1, perm).  Every value is moved as its bits (NaN payloads, -0 and denormals too).
 *
 * This reproduces what the trainer does and corrects nothing: a rotation by 180 degrees without a swap of the colours is not a
 * symmetry of chess (pawns then move the wrong way, and the side to move, castling and counter planes stay), and the mirror of the
 * files is a symmetry only for positions without castling rights (the castling planes are not swapped with the files). */
#ifndef M0_AUGMENT_H
#define M0_AUGMENT_H
#ifdef __cplusplus
extern "C" {
#endif

#define M0_AUG_NONE 0
#define M0_AUG_HFLIP 1
#define M0_AUG_ROT180 2

/* The kernel alone, on host arrays: planes [B][P][8][8], pi [B][4672], legal_mask [B][4672] u8 (nullable, then mask_out is null too),
 * kinds [B] u8 (M0_AUG_*) -> planes_out, pi_out, mask_out of the same shapes; a row of kind M0_AUG_NONE is copied.  M0_ERR_INVALID,
 * with the outputs untouched: a null planes, pi, kinds, planes_out or pi_out, B <= 0, P <= 0, a kind > 2, a mask without mask_out or
 * mask_out without a mask, an output that is its own input. */
int m0_augment_rows(int hip_device, const float* planes, int P, const float* pi, const uint8_t* legal_mask, const uint8_t* kinds, int B,
                    float* planes_out, float* pi_out, uint8_t* mask_out);
/* m0_net_score (m0_score.h) on the rows as kinds [B] u8 transforms them: one upload, the transform on the device into a second set of
 * staging buffers, the forward on the transformed planes, the same score kernel on the transformed pi and mask.  The argument checks
 * and M0_ERR_NONFINITE of m0_net_score; also M0_ERR_INVALID for a null kinds or a kind > 2, with `rows` untouched. */
int m0_net_score_aug(m0_net* net, const float* planes, const float* pi, const float* z, const uint8_t* legal_mask, const uint8_t* kinds,
                     int B, const m0_score_opts* opts, float* rows);
/* augment_rows_kernel alone on resident synthetic inputs of B rows (19 planes, with a mask, kinds 0, 1, 2 in turn), `iters` launches
 * between two events after one warm-up: *us_per_launch, and *bytes_per_launch = the bytes a launch must move, read and written
 * (tools/bench_augment.py). */
int m0_augment_bench(int hip_device, int B, int iters, float* us_per_launch, double* bytes_per_launch);

#ifdef __cplusplus
}
#endif
#endif /* M0_AUGMENT_H */
