/* A resident store of packed training rows and the batches a trainer reads from it (m0_engine.h includes this file: the calls
 * here are part of the same C ABI and the same library).  Packed rows (m0_rowpack.h) are appended segment by segment and stay in
 * device memory; a batch names rows by their ids and one launch writes them dense, already transformed by the trainer's
 * augmentation (m0_augment.h), into the caller's device memory: planes f32 [B][19][8][8], pi f32 [B][4672], z f32 [B] and
 * legal_mask u8 [B][4672].  Output row b of source row r and kind k is bit for bit
 *     m0_rowpack_unpack(r)  ->  m0_augment_rows(kind k)
 * and depends on (r, k) alone: not on B, on b or on the other rows.  Only the row ids and kinds cross from the host per batch.
 *
 *   ids       the rows of an append get first_row .. first_row + n - 1; ids ascend over the life of a store and are never reused.
 *   segments  one append is one segment (one allocation); eviction drops whole oldest segments.
 *   masks     a store is made for rows with masks or for rows without; a segment of the other sort is refused.
 *   host      a store created with hip_device -1 keeps its segments in host memory and fills batches with the same per-row code on
 *             the CPU (outputs_on_device must be 0): a machine without a GPU reads a store too. */
#ifndef M0_BATCH_H
#define M0_BATCH_H
#ifdef __cplusplus
extern "C" {
#endif

#define M0_ROWSTORE_HOST (-1)
/* m0_rowstore_info writes this many int64: resident rows, the first resident id (the next id when nothing is resident), the next
 * id, resident segments, resident RAW rows, bytes of the resident segments. */
#define M0_ROWSTORE_INFO 6

typedef struct m0_rowstore m0_rowstore;

/* hip_device >= 0: rows in that device's memory; M0_ROWSTORE_HOST: rows in host memory.  with_mask: rows carry masks (non-zero) or
 * not.  NULL on failure (m0_last_error). */
m0_rowstore* m0_rowstore_create(int hip_device, int with_mask);
void m0_rowstore_destroy(m0_rowstore* store);
/* The arrays are checked exactly as m0_rowpack_unpack checks them and uploaded as one segment; *first_row is the id of its first
 * row.  M0_ERR_INVALID for arrays that fail the checks or rows whose masks are not the store's sort; on any refusal nothing of
 * the store changes. */
int m0_rowstore_append(m0_rowstore* store, const m0_rowpack_arrays* in, int64_t* first_row);
/* Drops whole oldest segments while at least keep_rows rows stay resident (keep_rows 0 empties the store).  Every batch enqueued
 * before the call has finished before a segment is freed. */
int m0_rowstore_evict(m0_rowstore* store, int64_t keep_rows);
/* info i64 [M0_ROWSTORE_INFO] */
int m0_rowstore_info(m0_rowstore* store, int64_t* info);
/* rows i64 [B]: resident ids, duplicates allowed.  kinds u8 [B]: M0_AUG_* per row, NULL for M0_AUG_NONE everywhere.  mask is
 * required exactly when the store has masks.  outputs_on_device 1: the outputs are device memory of the store's device, 16-byte
 * aligned; the work is enqueued on `stream` (a hipStream_t, NULL the default stream) and the call does not wait for it.
 * outputs_on_device 0: the outputs are host memory and are filled when the call returns (stream is ignored).  M0_ERR_INVALID with
 * no output byte written: an id that is not resident (the message names it), a kind > 2, a missing or superfluous mask, B <= 0,
 * a null rows, planes, pi or z, device outputs of a host store.  After the first batch of a size no call allocates or frees. */
int m0_rowstore_batch(m0_rowstore* store, const int64_t* rows, const uint8_t* kinds, int B, float* planes, float* pi, float* z,
                      uint8_t* mask, int outputs_on_device, void* stream);
/* The same rows from the same per-row code on the CPU, over one set of packed arrays: rows i64 [B] index into `in`.  The arrays
 * are checked as m0_rowstore_append checks them. */
int m0_rowstore_batch_host(const m0_rowpack_arrays* in, const int64_t* rows, const uint8_t* kinds, int B, float* planes, float* pi,
                           float* z, uint8_t* mask);
/* Timing on resident rows, the rows of m0_rowpack_bench (every row PACKED with a LEGAL mask), kinds 0, 1, 2 in turn, rows taken in
 * a seeded shuffle: microseconds per batch of the fused kernel (*fused_us) and of the chain it replaces on the same rows in
 * order, encode + unpack + augment (*chain_us), each averaged over `iters` launches twice, the two kinds of launch alternating:
 * fused_us and chain_us are f32 [2], first and second run.  *dense_bytes: what a batch writes, B * 28 228. */
int m0_rowstore_bench(int hip_device, int B, int iters, float* fused_us, float* chain_us, double* dense_bytes);

#ifdef __cplusplus
}
#endif
#endif /* M0_BATCH_H */
