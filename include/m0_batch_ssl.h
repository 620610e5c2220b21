/* The SSL target maps of a batch read from a resident row store (m0_engine.h includes this file behind m0_batch.h: the calls here
 * are part of the same C ABI and the same library).  The trainer's loss is policy + value + ssl_weight * ssl_loss; a batch of
 * m0_rowstore_batch carries nothing for the third term, and the trainer would make the maps from the augmented planes with dozens
 * of small tensor operations per batch.  The calls here write them in the launch that writes the batch.
 *
 * For output row b of a batch (source row r, kind k), beside planes / pi / z / mask exactly as m0_rowstore_batch writes them:
 *   ssl[b]         f32 [17][64] in the layout of m0_game_record.ssl and m0_ssl_targets_fens (piece one-hot 13, threat, pin, fork,
 *                  control): bit for bit what m0_ssl_targets_planes gives for planes[b], the planes the same call writes.  The
 *                  maps are those of the TRANSFORMED planes, not transformed maps of the stored row: the reference's pawn attacks
 *                  point one way in tensor space, so under M0_AUG_ROT180 the two differ (under M0_AUG_HFLIP they agree).
 *   ssl_status[b]  i32: 0, or 1 for a row whose planes are not usable (m0_ssl_score.h).  Such a row gets all 17 maps written as
 *                  0 -- unlike m0_ssl_targets_planes, which leaves them alone: a batch writes every output byte exactly once.
 *                  A PACKED row is a position and always usable; only RAW rows can have status 1.
 * Both depend on (r, k) alone: not on B, on b or on the other rows. */
#ifndef M0_BATCH_SSL_H
#define M0_BATCH_SSL_H
#ifdef __cplusplus
extern "C" {
#endif

/* maps per row of ssl */
#define M0_BATCH_SSL_CH 17

/* m0_rowstore_batch with two more outputs: ssl f32 [B][M0_BATCH_SSL_CH][64] and ssl_status i32 [B], device memory (ssl on a
 * 16-byte boundary) or host memory as the other outputs.  Everything m0_rowstore_batch says about streams, eviction, host stores
 * and allocation holds here; M0_ERR_INVALID with no output byte written for everything it refuses and for a null ssl or
 * ssl_status. */
int m0_rowstore_batch_ssl(m0_rowstore* store, const int64_t* rows, const uint8_t* kinds, int B, float* planes, float* pi, float* z,
                          uint8_t* mask, float* ssl, int32_t* ssl_status, int outputs_on_device, void* stream);
/* m0_rowstore_batch_host with the same two outputs, from the same per-row code on the CPU. */
int m0_rowstore_batch_ssl_host(const m0_rowpack_arrays* in, const int64_t* rows, const uint8_t* kinds, int B, float* planes,
                               float* pi, float* z, uint8_t* mask, float* ssl, int32_t* ssl_status);
/* Timing on the rows of m0_rowstore_bench (every row PACKED with a LEGAL mask, kinds 0, 1, 2 in turn, rows in a seeded shuffle):
 * microseconds per batch of the launch with the maps (*fused_us) and of what it replaces on the same rows, the launch without
 * them followed by the targets kernel of m0_ssl_targets_planes on the planes it wrote (*chain_us), each averaged over `iters`
 * launches twice, the two sorts of launch alternating: fused_us and chain_us are f32 [2], first and second run.  *dense_bytes:
 * what a batch writes, B * (28 228 + 17 * 256 + 4). */
int m0_rowstore_bench_ssl(int hip_device, int B, int iters, float* fused_us, float* chain_us, double* dense_bytes);

#ifdef __cplusplus
}
#endif
#endif /* M0_BATCH_SSL_H */
