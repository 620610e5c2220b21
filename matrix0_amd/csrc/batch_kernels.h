// Launcher of batch_kernels.hip: a training batch gathered from resident packed rows, expanded and augmented in one launch
// (include/m0_batch.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "batch_core.h"

// refs [B] in device memory, each naming a row of a resident device segment (the host has checked row < n and kind <= 2) ->
// planes f32 [B][19][64], pi f32 [B][4672], z f32 [B], mask u8 [B][4672] (null: a store without masks), all device memory with
// planes, pi and mask on 16-byte boundaries.  One wave per output row; every byte of planes, pi and mask is written once.
hipError_t launch_batch_rows(const m0batch::RowRef* refs, int B, float* planes, float* pi, float* z, uint8_t* mask, hipStream_t st);
// The same launch with the SSL target maps of the output planes (include/m0_batch_ssl.h): ssl f32 [B][17][64] and ssl_status
// i32 [B], device memory, each map stored as one 256-byte row by the wave of its output row; the other outputs bit for bit those
// of launch_batch_rows.
hipError_t launch_batch_rows_ssl(const m0batch::RowRef* refs, int B, float* planes, float* pi, float* z, uint8_t* mask, float* ssl,
                                 int32_t* ssl_status, hipStream_t st);
