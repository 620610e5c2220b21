// Launcher of score_rows_kernel (score_kernels.hip) for the C-ABI units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/m0_engine.h"

// All pointers are device memory; legal_mask may be null unless opts.mask_mode is M0_SCORE_MASK_LEGAL.  logits, pi and rows are
// 16-byte aligned, legal_mask 4-byte aligned (what hipMalloc gives); B > 0.
hipError_t launch_score_rows(const float* logits, const float* value, const float* pi, const float* z, const uint8_t* legal_mask,
                             int B, const m0_score_opts& opts, float* rows, hipStream_t stream);
