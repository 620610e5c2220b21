// Launchers of rowpack_kernels.hip (include/m0_rowpack.h): dense rows <-> packed rows on the device, one wave per row.  All
// pointers are device memory; n <= 0 launches nothing.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/m0_engine.h"
#include "chess_core.h"

// Pass 1 of packing, behind launch_decode_planes (tree.h) on the same rows: pos / status are what the decode left.  Writes the
// row's m0_rowpack_pos (its kinds included) and counts i32 [n][2]: the pi entries and the LIST mask entries the row will store
// (both 0 for a RAW row).  mask may be null; so may pi (rows without a policy: no entries, zero raw_pi rows).
hipError_t launch_rowpack_count(const float* pi, const uint8_t* mask, const m0::Pos* pos, const int32_t* status, int n,
                                m0_rowpack_pos* out_pos, int32_t* counts, hipStream_t st);
// Pass 2: pi_off / mask_off i64 [n + 1] are the exclusive scans of the counts, raw_slot i32 [n] the RAW rows' places in the raw
// arrays (unread for PACKED rows).  Every row writes only its own ranges.
hipError_t launch_rowpack_fill(const float* planes, const float* pi, const uint8_t* mask, const m0_rowpack_pos* pos,
                               const int64_t* pi_off, const int64_t* mask_off, const int32_t* raw_slot, int n, uint16_t* pi_idx,
                               float* pi_val, uint16_t* mask_idx, float* raw_planes, float* raw_pi, uint8_t* raw_mask, hipStream_t st);
// The way back, behind launch_encode_positions on the rows' positions (which wrote every row's planes and, with a mask, its legal
// moves): dense pi of every row, the masks of LIST rows, and planes, pi and mask of RAW rows from the raw arrays.  mask null for
// rows without masks.  The entries must have been checked (capi_rowpack.hip: check_arrays).
hipError_t launch_rowpack_unpack(const m0_rowpack_pos* pos, const int64_t* pi_off, const uint16_t* pi_idx, const float* pi_val,
                                 const int64_t* mask_off, const uint16_t* mask_idx, const int32_t* raw_slot, const float* raw_planes,
                                 const float* raw_pi, const uint8_t* raw_mask, int n, float* planes, float* pi, uint8_t* mask,
                                 hipStream_t st);
