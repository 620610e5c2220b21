/* Packed training rows ("rowpack"; m0_engine.h includes this file: the calls here are part of the same C ABI and the same
 * library).  A stored row is s f32 [19][64], pi f32 [4672], legal_mask u8 [4672] (optional) and z: 28 228 bytes.  What it says is
 * small: twelve bitboards, a few scalars, the non-zero entries of pi and a mask that nearly always equals the legal moves of the
 * position.  The packed form keeps exactly that, and nothing is ever lossy: a row that the packed form cannot give back bit for
 * bit stays dense in side arrays.
 *
 *   row kinds   PACKED when the planes -> position decode (m0_decode_planes) gives M0_DECODE_OK or M0_DECODE_MASK_MISMATCH --
 *               the planes then re-encode bit for bit, which the decoder has verified (a saturated counter too: 99 re-encodes
 *               to exactly 1.0) -- and the mask, where given, holds only 0 and 1.  Everything else is RAW.
 *   mask kinds  NONE: the source had no mask (all rows of a call or none).  LEGAL: the mask equals the legal moves of the
 *               position, chosen exactly when the decoder reports no mismatch.  LIST: the set columns, explicitly.  A RAW row
 *               with a mask says LIST and keeps the mask dense.
 *   pi          CSR over the rows: pi_off i64 [n + 1], pi_idx u16 and pi_val f32 in ascending column order.  A column is an
 *               entry if and only if the float's BIT PATTERN is not 0x00000000: -0.0, denormals and NaN payloads are entries and
 *               come back bitwise.  0 .. 4672 entries per row; RAW rows have none (their pi is dense in raw_pi).
 *   LIST masks  CSR of u16 in the same way (mask_off, mask_idx); rows of another mask kind, and RAW rows, have no entries.
 *   RAW rows    the r-th RAW row in row order has its planes, pi and mask (with a mask) verbatim in row r of raw_planes
 *               f32 [19 * 64], raw_pi f32 [4672], raw_mask u8 [4672].
 *   z           carried as it is.
 *
 * Unpacking a PACKED row makes a position of the packed one and runs the engine's own encoder (m0_encode_fens' kernel) for the
 * planes and a LEGAL mask: there is no second decoder and no second encoder. */
#ifndef M0_ROWPACK_H
#define M0_ROWPACK_H
#ifdef __cplusplus
extern "C" {
#endif

#define M0_ROWPACK_VERSION 1

#define M0_ROWPACK_PACKED 0
#define M0_ROWPACK_RAW    1

#define M0_ROWPACK_MASK_NONE  0
#define M0_ROWPACK_MASK_LEGAL 1
#define M0_ROWPACK_MASK_LIST  2

/* One row's position, 104 bytes.  men: the twelve piece planes as bitboards in plane order (white P N B R Q K, black P N B R Q K),
 * a1 = bit 0, h8 = bit 63.  turn: 1 white to move.  castling: the four CLEANED rights as the planes hold them, bit 0 white
 * king side, 1 white queen side, 2 black king side, 3 black queen side.  ep: the en-passant square as the decoder found it in the
 * mask (a1 = 0), 255 none.  halfmove 0 .. 99 and fullmove 0 .. 199: the planes' counters as integers (the caps mean "or more").
 * A RAW row has row_kind M0_ROWPACK_RAW, its mask kind, and zeros elsewhere. */
typedef struct m0_rowpack_pos {
    uint64_t men[12];
    uint8_t turn, castling, ep, halfmove, fullmove, row_kind, mask_kind, reserved;
} m0_rowpack_pos;

/* The arrays of n packed rows, in the caller's memory (host pointers).  pi_n, mask_n and raw_n say how many entries resp.
 * rows the arrays behind them hold: for m0_rowpack_pack* the caller's capacities on entry, for every other call the counts.
 * An array of no entries (mask_idx with mask_n 0, the raw arrays with raw_n 0) may be NULL; the others are required. */
typedef struct m0_rowpack_arrays {
    int64_t n, pi_n, mask_n, raw_n;
    m0_rowpack_pos* pos;        /* [n] */
    float* z;                   /* [n] */
    int64_t* pi_off;            /* [n + 1] */
    uint16_t* pi_idx;           /* [pi_n] */
    float* pi_val;              /* [pi_n] */
    int64_t* mask_off;          /* [n + 1] */
    uint16_t* mask_idx;         /* [mask_n] */
    float* raw_planes;          /* [raw_n][19 * 64] */
    float* raw_pi;              /* [raw_n][4672] */
    uint8_t* raw_mask;          /* [raw_n][4672]; NULL without masks */
} m0_rowpack_arrays;

/* Dense rows -> packed rows on the device (one wave per row; a count pass, a scan of the counts on the host, a fill pass).
 * planes f32 [n][19][64], pi f32 [n][4672] or NULL (rows without a policy pack with no entries, as rows of zeros do: a caller that
 * knows the entries, such as one move per row, writes them itself), z f32 [n], legal_mask u8 [n][4672] or NULL.  sizes i64 [3] is written FIRST: the pi
 * entries, the LIST mask entries and the RAW rows that these rows need.  When out->pi_n, out->mask_n or out->raw_n is smaller
 * than that (or an array that would be written is NULL) the call returns M0_ERR_INVALID with sizes set and nothing else written;
 * otherwise the arrays are filled and the three counts in `out` are set to the sizes.  The output of a row does not depend on
 * n, on the row's index or on a repetition.  M0_ERR_HIP without a device. */
int m0_rowpack_pack(int hip_device, const float* planes, const float* pi, const float* z, const uint8_t* legal_mask, int n,
                    m0_rowpack_arrays* out, int64_t* sizes);
/* Packed rows -> dense rows on the device, out of place: planes f32 [n][19][64], pi f32 [n][4672], z f32 [n] and legal_mask
 * u8 [n][4672] (NULL for rows without masks; M0_ERR_INVALID when rows of mask kind NONE meet a mask output or the other way
 * round).  The arrays are checked before anything is written: offsets that do not ascend from 0 to the counts, columns that are
 * not ascending inside a row or not below 4672, kinds out of range, fields of a position out of range, fewer RAW rows than
 * raw_n says are M0_ERR_INVALID. */
int m0_rowpack_unpack(int hip_device, const m0_rowpack_arrays* in, float* planes, float* pi, float* z, uint8_t* legal_mask);
/* The same two results from the same per-row code on the CPU, with no device: a reader on a machine without a GPU still works. */
int m0_rowpack_pack_host(const float* planes, const float* pi, const float* z, const uint8_t* legal_mask, int n,
                         m0_rowpack_arrays* out, int64_t* sizes);
int m0_rowpack_unpack_host(const m0_rowpack_arrays* in, float* planes, float* pi, float* z, uint8_t* legal_mask);

/* m0_net_score (m0_score.h) of packed rows: the packed arrays are uploaded, unpacked on the network's device and stream into the
 * very staging buffers that m0_net_score fills from dense host arrays, and then m0_net_score's launches run: `rows` equals
 * m0_net_score's of the dense rows bit for bit.  RAW rows ride along dense.  M0_SCORE_MASK_LEGAL needs rows with masks. */
int m0_net_score_packed(m0_net* net, const m0_rowpack_arrays* in, const m0_score_opts* opts, float* rows);

/* Timing on resident rows, as m0_score_bench: B positions from seeded legal play, soft pi on about two thirds of each one's legal
 * moves, the legal moves as mask (every row PACKED with a LEGAL mask).  Microseconds per launch set of packing (decode, count,
 * fill) and of unpacking (encode, expand) averaged over `iters`, and the dense bytes a set reads resp. writes: B * 28 224. */
int m0_rowpack_bench(int hip_device, int B, int iters, float* pack_us, float* unpack_us, double* dense_bytes);

#ifdef __cplusplus
}
#endif
#endif /* M0_ROWPACK_H */
